// f2v_engine.hip -- HBM-resident Force2Vec engine behind the C ABI of include/f2v.h.
//
// Device layout (all in the HBM of one MI355X):
//   X[2]       fp32 [(N+pad) x D] row-major (rows 4*D bytes apart: 512 B at D = 128): the current matrix and
//              the one this epoch's new rows are written to; they swap when an epoch completes
//   rowptr     u32  [N+1], colids u32 [nnz]           (the reference's CSR, sample/CSR.h:89-96)
//   partials   fp32 [hub chunks x D]  partial force sums of split hub rows
//   sample ids u32, walks u32 [5N], sigmoid table fp32 [2048]
// The host side only sequences launches; every arithmetic step runs in f2v_kernels.hip.h.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>  // f2v_ranking sorts its keys with it

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <condition_variable>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <atomic>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "f2v.h"
#ifdef F2V_TEST_HOOKS
#include "f2v_test.h"
#endif
#include "f2v_internal.h"
#include "f2v_kernels.hip.h"
#include "f2v_nearest.hip.h"
#include "f2v_kmeans.hip.h"
#include "f2v_index.hip.h"
#include "f2v_logreg.hip.h"
#include "f2v_separation.hip.h"
#include "f2v_layout.hip.h"
#include "f2v_exact.hip.h"
#include "f2v_foldin.hip.h"
#include "f2v_linkpairs.hip.h"
#include "f2v_heldout.hip.h"
#include "f2v_neighbourhood.hip.h"
#include "f2v_pairranks.hip.h"
#include "f2v_louvain.hip.h"
#include "f2v_components.hip.h"
#include "f2v_tsne.hip.h"

using namespace f2v;

#define HIPC(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(e__ == hipErrorOutOfMemory ? F2V_ENOMEM : F2V_ENODEV, "%s: %s (%s:%d)", #expr,  \
                        hipGetErrorString(e__), __FILE__, __LINE__);                                   \
    } while (0)

constexpr size_t kIpcMaxBytes = (size_t)1 << 31;  // allocations of this size and more cannot be opened through HIP IPC (f2v_push_export)
constexpr uint32_t kPadRows = 4096;  // slack behind row N for the padded in-place all-gather of the last minibatch
constexpr int kMaxFinLevels = 32;  // fan-in >= 2: 2^32 chunks
constexpr uint32_t kLossLogMax = 4096;  // "loss_every": entries one f2v_train keeps
struct Plan {
    size_t item_off = 0;
    uint32_t n_items = 0, n_hubs = 0, n_chunks = 0, n_slots = 0;
    int n_levels = 0;  // levels of the hub combine trees
    size_t fin_off[kMaxFinLevels] = {};
    uint32_t fin_cnt[kMaxFinLevels] = {};
    uint64_t nnz = 0;
    uint64_t compulsory = 0;  // bytes this launch must move even with perfect caching inside the launch ("count_compulsory")
};

// The resident plan arrays reach gigabytes (RMAT-24 at batch 384: 2.9 GB) and are filled by memcpy from the parts the host's threads
// built: resize() must not zero them first (one thread, page by page) -- an allocator whose construct() of no arguments default-initialises.
template <class T>
struct RawInit : std::allocator<T> {
    template <class U> struct rebind { using other = RawInit<U>; };
    using std::allocator<T>::allocator;
    template <class U> void construct(U *p) noexcept { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
template <class T> using PlanVec = std::vector<T, RawInit<T>>;

struct SeenScratch {  // "count_compulsory": has this row been counted in this minibatch?  One stamp per vertex (a plan-building thread owns one)
    std::vector<uint32_t> seen;
    uint32_t stamp = 0;
};

// One launch of qstep_chain_kernel: up to 64 consecutive minibatches (f2v_kernels.hip.h, "chained minibatches")
struct ChainPlan {
    size_t item_off = 0, fin_off = 0, wg_off = 0;
    uint32_t n_wgs = 0, n_batches = 0, n_slots = 0, n_fin = 0;
    uint32_t first_batch = 0;  // global minibatch index of its first minibatch
    uint32_t lo = 0, hi = 0, last_lo = 0;   // rows covered; first row of the last minibatch
    uint64_t nnz = 0, compulsory = 0;
    uint32_t n_hubs = 0, n_chunks = 0;
};

// One launch of qwide_chain_kernel: the same minibatches as workgroup PROGRAMS (f2v_kernels.hip.h, "wide form")
struct WidePlan {
    size_t item_off = 0, fin_off = 0, wg_off = 0, job_off = 0;
    uint32_t n_wgs = 0, n_batches = 0, n_slots = 0;
    uint32_t first_batch = 0;
    uint32_t lo = 0, hi = 0, last_lo = 0;
    uint64_t nnz = 0, compulsory = 0;
    uint32_t n_hubs = 0, n_chunks = 0;
    uint32_t n_helpers = 0, n_finishers = 0, n_packed = 0, n_node_wgs = 0;  // workgroups by role
    uint32_t width = 0;  // the sub-wave layout its programs are laid out for (wide_width)
};

// what a rank hands its peers (f2v_push_export): F2V_PUSH_EXPORT_BYTES bytes
struct PushExport {
    hipIpcMemHandle_t x[2], flags;  // landing-buffer mode: x[0] is the landing buffer, x[1] unused
    uint32_t magic, n, D, cur;
    uint32_t landing, landing_cap;
    char bus_id[16];  // PCI bus id of the exporting rank's GPU: ranks that share a card run without "piece_affinity"
    uint32_t caps;    // bit 0: this rank's GPU starts workgroups XCD-round-robin in index order (what chained launches count on)
    char reserved[F2V_PUSH_EXPORT_BYTES - 3 * sizeof(hipIpcMemHandle_t) - 28 - 16];
};
static_assert(sizeof(PushExport) == F2V_PUSH_EXPORT_BYTES, "export blob layout");
static_assert(kMaxRanks == F2V_PUSH_MAX_RANKS, "rank limit");
constexpr uint32_t kPushMagic = 0x46325650u;  // "F2VP"

// ---- what the host code shares: the owners of device memory, pinned memory and events, the resident plan arrays,
// and (further down) settled_enter and allow_lds.  New host code uses these, it does not bring its own.
#define F2VC(expr)                        \
    do {                                  \
        int rc__ = (expr);                \
        if (rc__ != F2V_OK) return rc__;  \
    } while (0)

// A device array and the elements it holds: allocated on first use, grown (never shrunk, never rounded up) for a larger call, freed
// with its owner -- the handle (f2v_destroy has made the handle's device current by then) or the call whose local it is
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    // Room for `count` elements.  Growing waits for the handle's stream first (launches may still read the old array) and leaves the
    // buffer empty where the allocation fails: "<what> workspace: <hip error>".
    int reserve(f2v_ctx *c, size_t count, const char *what);
    // ... without a handle (a local of a call that takes a device number) or behind a wait the caller has made: no stream is waited for.
    // `finegrained`: memory whose stores the peers of the push exchange see while a kernel runs (the flags)
    int reserve(size_t count, const char *what, bool finegrained = false) {
        if (p && cap >= count) return F2V_OK;
        const hipError_t e = grow(count, finegrained);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? F2V_ENOMEM : F2V_ENODEV, "%s workspace: %s", what, hipGetErrorString(e));
        return F2V_OK;
    }
    // ... for a buffer the call can do without: did the device have room?  No error text is left behind.
    bool try_reserve(size_t count) {
        if (p && cap >= count) return true;
        if (grow(count, false) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }

private:
    hipError_t grow(size_t count, bool finegrained) {  // the capacity is set where the allocation succeeded, and only there
        release();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        const hipError_t e = finegrained ? hipExtMallocWithFlags((void **)&p, bytes, hipDeviceMallocFinegrained) : hipMalloc((void **)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = count;
        return e;
    }
};

// A pinned host array: what asynchronous copies read and write while the host goes on
template <class T>
struct HostBuf {
    T *p = nullptr;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { release(); }
    operator T *() const { return p; }
    int reserve(size_t count) {  // once: a pinned array is never grown
        if (!p) HIPC(hipHostMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
        return F2V_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
};

// A set of events, destroyed together: on every way out of the function whose local it is
struct DevEvents {
    std::vector<hipEvent_t> all;
    DevEvents() = default;
    DevEvents(const DevEvents &) = delete;
    DevEvents &operator=(const DevEvents &) = delete;
    ~DevEvents() { release(); }
    int make(hipEvent_t *e, unsigned flags = hipEventDefault) {
        hipEvent_t made = nullptr;
        HIPC(hipEventCreateWithFlags(&made, flags));
        all.push_back(*e = made);
        return F2V_OK;
    }
    void release() {
        for (hipEvent_t e : all) (void)hipEventDestroy(e);
        all.clear();
    }
};

// Device time between two points of a stream: start, stop, and -- once the stream has been synchronised -- seconds
struct DevTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    DevEvents made;
    int start(hipStream_t stream) {
        for (hipEvent_t &e : ev)
            if (!e) F2VC(made.make(&e));
        HIPC(hipEventRecord(ev[0], stream));
        return F2V_OK;
    }
    int stop(hipStream_t stream) {
        HIPC(hipEventRecord(ev[1], stream));
        return F2V_OK;
    }
    int seconds(double *sum) {  // *sum += the seconds from start to stop
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *sum += ms * 1e-3;
        return F2V_OK;
    }
};

// One of the launch plans' arrays: the host's copy, which the planners append to, the device's, and how many elements of it are resident
template <class T>
struct PlanArray {
    PlanVec<T> h;
    DevBuf<T> d;
    size_t resident = 0;
    // Make everything appended so far resident (the caller has waited for the launches that read the array): an array that has
    // outgrown the device's is given half as much again, at least `floor` elements, and copied whole; otherwise only its new tail is.
    int upload(size_t floor) {
        if (h.size() > d.cap) {
            resident = 0;
            F2VC(d.reserve(std::max<size_t>(h.size() * 3 / 2, floor), "launch plan"));
        }
        if (h.size() > resident) HIPC(hipMemcpy(d + resident, h.data() + resident, (h.size() - resident) * sizeof(T), hipMemcpyHostToDevice));
        resident = h.size();
        return F2V_OK;
    }
    void clear() {  // the device's array keeps its capacity
        h.clear();
        resident = 0;
    }
    size_t bytes() const { return h.size() * sizeof(T); }
};

struct f2v_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n = 0, D = 0;
    uint64_t nnz = 0;
    int vec = 1;
    bool exact = false;
    std::vector<uint32_t> rowptr, colids;  // host copies: hub planning, walk generation, statistics
    DevBuf<uint32_t> d_rowptr, d_colids, d_ids;
    DevBuf<uint32_t> d_walk_buf[2];  // two walk buffers: f2v_train (option 7) alternates between them, epoch by epoch
    uint32_t *d_walks = nullptr;     // ... and the one that holds the current walks (not an owner)
    size_t ids_valid = 0;  // prefix of d_ids uploaded by f2v_upload_sample_ids
    DevBuf<float> d_X[2], d_partials, d_table;  // (d_X: allocated once, by f2v_create -- their addresses are exported)
    DevBuf<uint32_t> d_ready, d_kerr;  // combine-tree flags (one per partial slot), kernel error word
    uint32_t launch_seq = 0;
    uint32_t xcc_count = 0;      // XCDs seen by the dispatch probe of f2v_create
    bool xcc_round_robin = false;  // ... and workgroup b ran on the XCD of workgroup b mod 8
    int64_t tree_timeout_ms = 5000;
    int64_t chain_timeout_ms = 200;  // chained launches: a healthy one lasts a millisecond or two, so a lost one is noticed in milliseconds
    // f2v_train survives a give-up ("recover"): the matrix and the rand() state as they were when the call began
    bool recover = true;
    DevBuf<float> d_snap;
    DevTimer snap_timer;  // around the snapshot copy: f2v_stats.snapshot_seconds
    // in-grid waits that were switched off by a RECOVERED give-up come back by themselves: after `waits_backoff` healthy f2v_train
    // calls (1, then 2, 4 ... 64: a card that keeps losing launches is asked less and less often); a give-up that was not recovered
    // from, the dispatch probe's verdict and the caller's own "merge_finalize" = 0 stay
    bool waits_suspended = false;
    uint32_t waits_backoff = 1, calls_since_give_up = 0;
    uint32_t recoveries = 0;
    bool unit_degi = false;  // the option being run is 10 (StepArgs::unit_degi): set by every entry point that takes an option
    uint32_t mark_every = 0;       // "epoch_marks"
    std::vector<double> marks;     // f2v_train_marks
    // the training objective (f2v_objective, "loss_every"): row-piece items (built once, from rowptr alone), one ObjPartial per
    // workgroup, and the results -- slot k < kLossLogMax: entry k of f2v_train's log, slot kLossLogMax: f2v_objective's
    DevBuf<Item> d_obj_items;
    uint32_t obj_items = 0;
    DevBuf<ObjPartial> d_obj_part, d_obj_out;
    uint32_t loss_every = 0;                      // "loss_every"
    uint64_t loss_seed = 1;                       // "loss_seed"
    double last_loss_us = 0.0;                    // "last_loss_us"
    std::vector<uint32_t> loss_epochs;            // f2v_train_losses
    std::vector<double> loss_values;              // ... loss, attraction, repulsion per entry
    // nearest-neighbour queries (f2v_nearest_rows / _vectors, f2v_neighbour_recall): buffers of one query chunk, allocated on first
    // use and grown on demand; "nearest_splits" (0 = from nq and N), "nearest_block" (0 = from D and nq | 32 | 128), "nearest_chunk"
    struct Nearest {
        DevBuf<float> d_Q, d_rq, d_rc, d_scores;
        DevBuf<uint32_t> d_qids, d_ids;
        DevBuf<unsigned long long> d_ws, d_counts;
        DevTimer timer;
        uint32_t splits = 0, block = 0, chunk = 8192;
    } nn;
    // nearest neighbours through an index (f2v_index_*): the index in buffers of its own -- labels, members in list order, lists + 1
    // offsets, centroids; no scorer's workspace overlaps them -- and the buffers of one query chunk of a search, allocated on first
    // use and grown on demand; "index_chunk": queries per launch, "index_split_tiles": tiles of 128 candidates per work item of the
    // scan (a longer list is cut into several ranges), "index_block" (0 = 128 where D <= 128 and a bucket has more than 32 queries
    // left, else 32 | 32): queries per work item -- placement only
    struct Index {
        DevBuf<uint32_t> d_labels, d_members, d_offsets;
        DevBuf<float> d_C;
        std::vector<uint32_t> offsets;  // host copy of d_offsets
        f2v_index_t info{};
        bool built = false;
        DevBuf<float> d_Q, d_rq, d_rc, d_scores;
        DevBuf<uint32_t> d_qids, d_probes, d_counts, d_start, d_bucket, d_ids;
        DevBuf<IxItem> d_items;
        DevBuf<unsigned long long> d_ws;
        DevTimer timer;
        uint32_t chunk = 8192, split_tiles = 8, block = 0;
    } ix;
    int rows_sorted = -1;  // the CSR's ids ascend inside every row (rows are searched by the nearest queries and f2v_modularity): -1 not checked yet (rows_ascending)
    // clustering (f2v_kmeans, f2v_modularity): the workspace f2v.h states, allocated on first use for the call's k and grown for a
    // larger one; "kmeans_block" (0 = from k | 64 | 128 | 256): rows per workgroup of kmeans_assign_kernel
    struct Kmeans {
        DevBuf<float> d_C, d_bestC, d_dist;
        DevBuf<uint32_t> d_labels, d_bestL, d_order, d_hist, d_counts, d_start, d_pstart, d_changed, d_seed, d_mlabels;
        DevBuf<double> d_psum, d_ipart, d_inertia;
        DevBuf<unsigned long long> d_tallies;
        DevTimer timer;
        uint32_t block = 0;
    } km;
    // logistic regression (f2v_logreg_*): the workspace f2v.h states, allocated on first use and grown for a larger call
    struct Logreg {
        DevBuf<uint32_t> d_a, d_b, d_cmap;
        DevBuf<uint8_t> d_y;
        DevBuf<double> d_W, d_sums, d_part, d_z;
        DevTimer timer;
    } lr;
    // separation (f2v_silhouette, f2v_davies_bouldin): beside the clustering workspace (the counting sort, the centroids, the piece
    // sums) the buffers f2v.h states, allocated on first use and grown for a larger call; "separation_chunk": samples per launch,
    // "separation_block" (0 = 64 | 64 | 128): sample rows per workgroup of separation_pair_kernel
    struct Separation {
        DevBuf<uint32_t> d_ids, d_sid, d_slab, d_other, d_span_start, d_span_cnt, d_cspan;
        DevBuf<double> d_ws, d_s, d_part, d_S, d_sum;
        DevTimer timer;
        uint32_t chunk = 8192, block = 0;
    } sep;
    // layout (f2v_pca, f2v_trustworthiness): the buffers f2v.h states, allocated on first use and grown for a larger call;
    // "trust_chunk": samples per launch, "trust_block" (0 = 64 | 64 | 128): sample rows per workgroup of trust_rank_kernel
    struct Layout {
        DevBuf<double> d_ws, d_mean, d_S, d_W;
        DevBuf<float> d_P, d_Y;  // the projection, the caller's second matrix
        DevBuf<uint32_t> d_sid, d_nx, d_ny, d_hist;
        DevBuf<unsigned long long> d_thr, d_pen, d_sums;
        DevTimer timer;
        uint32_t chunk = 8192, block = 0;
    } lay;
    // exact all-pairs Force2Vec (option 1: f2v_train, f2v_objective): the workspace f2v.h states, allocated on first use and grown for a
    // larger minibatch; "exact_rows" (0 = automatic | 4 | 8 | 16): rows per workgroup of exact_pair_kernel; "exact_epoch": the index
    // of the next call's first epoch (it fixes the step)
    struct Exact {
        DevBuf<float> d_ws;
        DevBuf<double> d_rows, d_piece;
        uint32_t rows = 0;
        uint32_t quarter_min = 1024;  // "exact_quarter_min"
        uint32_t last_rows = 0;       // "last_exact_rows"
        bool last_quarter = false;    // "last_exact_quarter"
        uint64_t epoch = 0;
    } ex;
    // fold-in (f2v_fold_in): the workspace f2v.h states, allocated on first use and grown for a larger call; "fold_chunk": vertices per
    // launch, "fold_resident" (-1 = automatic | 0): the form that keeps a workgroup's lists in LDS was measured slower and is not built
    struct Fold {
        DevBuf<uint32_t> d_rowptr, d_ids, d_order;
        DevBuf<float> d_in, d_out;
        DevTimer timer;
        uint32_t chunk = 65536;
        int resident = -1;
    } fold;
    // link prediction pairs (f2v_link_pairs): the workspace f2v.h states, allocated on first use and grown for a larger call;
    // "link_short_max": the most negatives of a vertex that one wavefront draws (longer lists take a workgroup and a table)
    struct Link {
        DevBuf<uint32_t> d_p, d_total, d_order, d_u, d_v, d_table;
        DevBuf<uint8_t> d_y;
        DevBuf<unsigned long long> d_offset, d_tile, d_sums, d_table_at;
        DevTimer timer;
        uint32_t short_max = 256;
    } link;
    // held-out link prediction (f2v_edge_split, f2v_pair_scores, f2v_ranking): the workspace f2v.h states, allocated on first use and
    // grown for a larger call; "pairs_chunk": pairs per upload and launch of f2v_pair_scores -- placement only
    struct Heldout {
        DevBuf<uint32_t> d_anchor, d_kept, d_q, d_total, d_zero, d_order, d_table, d_rowptr, d_colids, d_hu, d_hv, d_nu, d_nv;
        DevBuf<uint8_t> d_ny;
        DevBuf<unsigned long long> d_kept_at, d_held_at, d_neg_at, d_tile, d_sums, d_table_at;
        DevBuf<uint32_t> d_pu, d_pv;   // f2v_pair_scores: one chunk's ids
        DevBuf<float> d_ps;            // ... and scores
        DevBuf<double> d_scores, d_terms, d_blocks;  // f2v_ranking
        DevBuf<unsigned long long> d_keys[2], d_tallies;
        DevBuf<uint8_t> d_labels[2], d_sort;
        DevBuf<uint32_t> d_cum;
        DevTimer timer;
        uint32_t pairs_chunk = 1u << 20;
    } held;
    // neighbourhood scores of pairs (f2v_pair_neighbourhood): the workspace f2v.h states, allocated on first use and grown for a larger
    // call; d_deg holds d(u) once degrees_built; "neighbourhood_spread" (1 | 0): the pieces of a pair of several pieces are work items
    // of their own, or every pair is one wavefront's -- placement only
    struct Neighbourhood {
        DevBuf<uint32_t> d_deg, d_u, d_v, d_items_of, d_zero, d_piece_c;
        DevBuf<unsigned long long> d_offset, d_tile, d_sums, d_item;
        DevBuf<double> d_piece_aa, d_piece_ra, d_out;
        DevTimer timer;
        bool degrees_built = false;
        bool spread = true;
        uint64_t last_items = 0;  // "last_neighbourhood_items": the piece items of the last call
    } nb;
    // ranks of pairs (f2v_pair_ranks): the workspace f2v.h states, allocated on first use and grown for a larger call; "ranks_chunk":
    // pairs per launch, "ranks_splits" (0 = from the query blocks and the tiles): candidate ranges a query block's work is cut into --
    // placement only.  timer: [0] targets and gather, [1] the base counts, [2] the correction
    struct Ranks {
        DevBuf<uint32_t> d_u, d_v, d_greater, d_equal;
        DevBuf<float> d_t, d_Q, d_rc;
        DevBuf<PrankItem> d_item;
        DevBuf<unsigned long long> d_excluded;
        DevTimer timer[3];
        uint32_t chunk = 8192, splits = 0;
        double base_seconds = 0.0, correct_seconds = 0.0;  // "last_ranks_base_us", "last_ranks_correct_us": of the last call
    } pr;
    // communities (f2v_louvain, f2v_partition_agreement): the workspace f2v.h states, allocated on first use and grown for a larger call;
    // "louvain_short_max": the longest row of a unit that 16 lanes gather, "louvain_lds_slots": the largest table kept in LDS --
    // placement only.  rows_symmetric: -1 not checked yet (checked once per handle, on the device)
    struct Louvain {
        DevBuf<uint32_t> d_k[2], d_loop[2], d_rowbeg[2], d_rowend[2], d_cols[2], d_wts[2];  // a level's graph: level l in set l & 1
        DevBuf<uint32_t> d_c, d_next, d_tot, d_size, d_kept, d_newid, d_ccount, d_members, d_units, d_table, d_vlabel, d_tile, d_flag;
        DevBuf<uint32_t> d_a, d_b, d_cells;
        DevBuf<unsigned long long> d_table_at, d_sums, d_bins;
        DevBuf<double> d_pieces;
        DevTimer timer;
        uint32_t short_max = 32, lds_slots = 4096;
        int rows_symmetric = -1;
    } lv;
    // components, spanning forests and subgraphs (f2v_components, f2v_spanning_forest, f2v_edge_split_connected's forest flags,
    // f2v_subgraph): the workspace f2v.h states, allocated on first use and grown for a larger call; "forest_key_bits": the leading bits
    // of a key that the forest's order looks at (a diagnostic knob: small values force ties).  items_built: the pieces of the long rows
    // are on the device; flags_*: which forest d_flag holds (a split with the same seed reuses it)
    struct Components {
        DevBuf<uint32_t> d_L, d_P, d_size, d_sizes, d_kept, d_cnt, d_zero, d_rowptr, d_colids, d_newid;
        DevBuf<CcItem> d_items;
        DevBuf<unsigned long long> d_sums, d_best1, d_best2, d_forest[2], d_id_at, d_row_at, d_tile;
        DevBuf<uint8_t> d_flag, d_keep, d_sort;
        DevTimer timer;
        uint32_t nitems = 0, key_bits = 64;
        bool items_built = false, flag_valid = false;
        uint64_t flag_seed = 0;
        uint32_t flag_bits = 0;
        std::vector<double> round_seconds;  // f2v_forest_round_seconds
    } cc;
    double cc_subgraph_seconds = 0.0;  // "last_subgraph_us"
    // t-SNE layout (f2v_tsne_affinities, f2v_tsne): the workspace f2v.h states, allocated on first use and grown for a larger call;
    // "tsne_rows" (0 = automatic | 64 | 128 | 256): rows per workgroup of tsne_pair_kernel, "tsne_slices" (0 = automatic): spans per
    // workgroup of it -- placement only
    struct Tsne {
        DevBuf<float> d_G, d_dist, d_yf;  // the gathered rows, the neighbours' scores, yf twice
        DevBuf<uint32_t> d_sid, d_nbr, d_prow, d_pcol;
        DevBuf<double> d_cond, d_pval, d_state, d_ws, d_part, d_out;  // d_state: Y, update, gains; d_out: Z, then the KL values
        DevTimer timer;
        uint32_t rows = 0, slices = 0;
        std::vector<uint32_t> kl_iters;  // f2v_tsne_kl_log
        std::vector<double> kl_values;
    } ts;
    uint32_t last_wide_width = 0;  // the layout width of the last wide-form f2v_train ("last_wide_width")
    bool last_wide_early = false;  // ... and whether it ran the kernel's EARLY form ("last_wide_early")
    int last_train_form = 0;  // how the last f2v_train launched: 0 one launch per minibatch, 1 chained, 2 chained in the wide form ("last_train_form")
    bool plan_overflow = false;  // a launch plan needed more than 2^28 partial-sum slots (kItemSlotMask)
    HostBuf<uint32_t> h_kerr;  // pinned: the kernel error words as of the last completed epoch-end copy (train_impl)
#ifdef F2V_TEST_HOOKS
    struct Hooks {  // what include/f2v_test.h switches on (fill_hooks hands it to the launches)
        uint32_t withhold_slot = kNoSlot, withhold_row = kNoSlot;  // f2v_test_withhold_flag, f2v_test_withhold_row
        uint32_t chain_mode = 0;                 // f2v_test_chain_nowait's argument as given: bit 0 -- chained launches without their row waits (results are then wrong)
        DevBuf<unsigned long long> d_xcd;        // f2v_test_xcd_times (StepArgs::xcd_times)
        DevBuf<unsigned long long> d_stamps;     // f2v_test_stamps: 4 wall-clock words per row (StepArgs::stamps)
        uint32_t stub = 0;                       // f2v_test_interaction_stub (StepArgs::test_stub)
    } hooks;
#endif
    bool merge_fin = true, capturing = false;  // all combine-tree levels in one launch (not while a hipGraph is captured)
    int cur = 0;  // d_X[cur]: current matrix; d_X[cur^1]: receives the rows updated this epoch
    bool have_x = false, have_walks = false;
    bool x_invalid = false;  // a lost launch left the embeddings half-updated: they must be set or initialised again
    Rand rng;
    // work-item plans (one per distinct launch: row range x neighbour source), see plan_for()
    uint32_t chunk = 64, fanin = 32;
    bool chunk_auto = true;  // f2v_train / "hub_chunk_for_batch" pick the chunk from the batch size
    bool use_quarter = true;  // sub-wave kernel when D is a multiple of 4 up to 256
    std::map<std::tuple<uint32_t, uint32_t, int>, Plan> plans;
    // chained minibatches ("chain_batches"): one launch per group of minibatches of f2v_train
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, int>, ChainPlan> chains;  // (first minibatch, minibatches, batch size, walk samples instead of CSR neighbours)
    PlanArray<WgDesc> plan_wg;
    // ... in the wide form ("chain_wide", the default where the fan-in allows it): workgroup programs and their jobs
    std::map<std::tuple<uint32_t, uint32_t, uint32_t, int>, WidePlan> wides;
    PlanArray<WideDesc> plan_wide;
    PlanArray<WJob> plan_jobs;
    bool wide = true;
    uint32_t wide_max_batch = 2048;  // larger chained minibatches are throughput-bound: they keep the HBM form (tools/wide_sweep.py)
    uint32_t wide_rows = 262144;     // rows one launch of the wide form covers ("chain_rows" is the HBM form's)
    uint32_t wide_order = 0;    // workgroups of a minibatch: 0 helpers, finishers, packed rows; 1 helpers, packed, finishers; 2 packed, helpers, finishers
    uint32_t wide_phases = 1;   // phases (of 32 piece slots) a workgroup of small rows runs
    uint32_t wide_min_width = 0;   // "wide_min_width" (wide_width; 0: chosen from the graph and the batch)
    // "wide_epochs": up to this many EPOCHS of a small graph in one wide-form launch (WideArgs::wgs_per_epoch): ring of matrices, per-epoch
    // row flags / partial-sum slots / their flags; 0 = automatic (32 for graphs of up to 2 M nonzeros that fit one launch, else 1)
    uint32_t wide_epochs = 0, last_wide_epochs = 1;
    DevBuf<float> d_ring, d_ring_partials;
    DevBuf<uint32_t> d_ring_flags, d_ring_ready;
    uint32_t ring_epochs = 0;   // epochs the ring buffers are sized for
    bool ring_refused = false;  // the device had no room for them
    size_t ring_slots = 0;      // partial-sum slots per epoch they are sized for
    // "wide_single" (measurement only): the wide form also where a launch holds ONE minibatch -- nothing is handed on inside such a
    // launch, what is left of the form is "a split row's pieces meet in LDS" (no partial sums through HBM, no tree nodes below
    // fanin^2 pieces): the plain launch form's alternative for large minibatches, measured and rejected (profiles/r04_*)
    bool wide_single = false;
    // "replicate_small": f2v_train_sharded at a batch size f2v_train would run chained (the reference's default 384 is one) runs the WHOLE
    // epoch on every rank and exchanges nothing: such an epoch is one chain of row-to-row dependencies (1 432 hops of ~5 us at batch 256
    // on RMAT-20) that a hop over xGMI can only lengthen -- sharded with one launch and one barrier per minibatch it took 41 ms per epoch
    // at batch 384 on two ranks where one GPU takes 6.7.  Every rank holds the same matrix and the same rand() state before and after
    // (the chained forms are deterministic).  1 (default): where no peer shares this rank's GPU (waiting workgroups of two processes on
    // one card can starve each other: bounded and recovered, but slow); 2: always; 0: never.
    int replicate_small = 1;
    int wide_samples_early = -1;  // "wide_samples_early": StepArgs::samples_early; -1 = automatic (graphs of up to 2 M nonzeros: the launch is one dependency chain)
    uint32_t wide_rounds = 0;   // rounds per phase of such a workgroup (0: one for minibatches of up to 512 rows, else as many as fill the piece slots)
    uint32_t wide_span = 2;     // fan-in groups per helper workgroup
    uint32_t wide_finish = 4;   // fan-in groups the finisher workgroup keeps for itself (the ones that wait longest)
    DevBuf<uint32_t> d_rowflag;  // per row: sequence number of the chained launch that last wrote it
    bool chain = true;            // "chain_batches"
    uint32_t chain_max_batch = 4096, chain_rows = 65536;  // measured on RMAT-20 (tools/small_batch.py, tools/chain_sweep.py)
    PlanArray<Item> plan_items;
    PlanArray<FinItem> plan_hubs;  // the nodes of the combine trees
    size_t max_slots = 0;  // partial-sum slots the plans need (d_partials and d_ready hold at least as many)
    // rows [upd_lo, upd_hi) have been updated since the last swap/fold and live in d_X[cur^1]
    uint32_t upd_lo = 0, upd_hi = 0;
    bool pending = false;             // a minibatch has been stepped since the last flush
    uint32_t p_lo = 0, p_hi = 0;      // ... and this is it (multi-GPU exchange window)
    int waves_per_block = 4;
    bool fast_rng = false;        // non-parity mode: device-side init and option-7 walks (counter-based RNG)
    uint64_t fast_seed = 1, fast_epoch = 0;
    int rows_in_flight = 0;  // 0: the kernels' default (4 at D = 128 and 256, 8 below)
    bool class_cut = true;         // split rows are also cut where their neighbour ids cross into the next eighth of the id range (piece_cuts)
    bool piece_affinity = true;    // hub pieces are placed on the XCD that owns their neighbours' id range (see plan_for)
    bool last_replicated = false;  // the last f2v_train_sharded ran the whole epoch on this rank ("replicate_small")
    bool shared_card = false;      // a peer of the push exchange runs on the same GPU: placement goes back to same-XCD groups
    bool count_compulsory = false;  // plans also count their compulsory bytes (f2v_stats.compulsory_bytes; costs O(nnz) per new plan)
    SeenScratch seen_scratch;  // ... with this marker array
    bool use_graph = false;  // f2v_train replays one hipGraph per epoch parity instead of launching eagerly
    f2v_stats stats{};
    // multi-GPU push exchange (include/f2v.h): peers' matrices and flags mapped through HIP IPC
    struct Push {
        bool exported = false, attached = false, local = false;  // local: peers are handles of this process (self-test)
        uint32_t rank = 0, world = 1;
        float *peer_X[2][kMaxRanks] = {};
        DevBuf<unsigned long long> flags;  // fine-grained, a fresh array per f2v_push_export (its address is exported)
        unsigned long long *peer_flags[kMaxRanks] = {};
        DevBuf<uint32_t> d_err;
        unsigned long long seq = 0;
        int64_t timeout_ms = 20000;
        bool fused = true;  // rows are pushed by the step / finalize kernels themselves ("push_fused" = 0: by a kernel after them)
        // reader masks: neighbour part cached per (batch, world), sampled vertices patched in per run
        std::vector<uint32_t> base_masks, patched_ids;
        uint32_t mask_batch = 0, mask_world = 0;
        DevBuf<uint32_t> d_masks, d_patch;
        uint64_t pushed_per_epoch = 0, rows_pushed = 0, rows_allgather = 0;
        bool any_shared = false, all_chain = true;  // over all attached ranks (f2v_push_attach): "replicate_small"
        // Landing-buffer mode: hipIpcOpenMemHandle never returns for an allocation of 2 GiB or more (ROCm 7.x), so a
        // matrix that large cannot be mapped into the peers.  The peers then push a minibatch's rows into a small
        // mapped buffer (two halves, alternating per exchange) and unpack_rows_kernel moves them into the matrix
        // behind the barrier.
        bool landing = false, force_landing = false;
        DevBuf<float> landing_buf;  // a fresh one per f2v_push_export in this mode (its address is exported)
        float *peer_landing[kMaxRanks] = {};
        uint32_t landing_cap = 0;  // rows per half
        uint32_t round = 0;        // exchanges done: (round & 1) is the half in use
    } push;
};

template <class T>
int DevBuf<T>::reserve(f2v_ctx *c, size_t count, const char *what) {
    if (p && cap >= count) return F2V_OK;
    HIPC(hipStreamSynchronize(c->stream));
    return reserve(count, what);
}

namespace {

int pick_vec(uint32_t D) {
    int v = 1;
    while ((uint32_t)(64 * v) < D) v <<= 1;
    return v;
}

// Hub chunk for minibatches of `batch` rows: a chunk is one quarter-wave's serial stretch (one dependent
// round trip per group of U = 4 neighbours, whose rows are in flight together), the launch as a whole streams ~516 B
// per nonzero at ~6 TB/s; keeping the longest stretch at about half the launch's streaming time gives chunk ~ batch
// nonzeros / 14000 (measured optimum on RMAT-20: 16 at B=4096, 32 at B=16384, 128 at B=65536 -- measured while the
// step kernel still waited for each row before requesting the next, ~0.6 us per neighbour; not re-fitted since).  It depends only on
// the graph and the number of rows one launch covers (the batch, or a rank's slice of it in f2v_train_sharded).
uint32_t auto_chunk(const f2v_ctx *c, uint32_t batch) {
    const double est = (double)std::min(batch, c->n) * ((double)c->nnz / (double)c->n) / 14000.0;
    // (from 4: minibatches of up to ~2000 rows are bound by the latency of their longest item, not by throughput -- batch 256
    // chained: 15.6 ms per epoch with 4-neighbour pieces, 18.2 with 8, 23.6 with 16)
    uint32_t ch = 4;
    while (ch < 512 && (double)ch * 1.5 < est) ch <<= 1;
    return ch;
}

void drop_plans(f2v_ctx *c) {
    c->plans.clear();
    c->chains.clear();
    c->wides.clear();
    c->max_slots = 0;
    c->plan_wg.clear();
    c->plan_wide.clear();
    c->plan_jobs.clear();
    c->plan_items.clear();
    c->plan_hubs.clear();
}

int current_walks(f2v_ctx *c) {  // d_walks exists: the first walk buffer where none is current yet
    if (c->d_walks) return F2V_OK;
    F2VC(c->d_walk_buf[0].reserve((size_t)c->n * kWalkLength, "walks"));
    c->d_walks = c->d_walk_buf[0];
    return F2V_OK;
}

// Width of the sub-wave layout that serves this D -- the smallest of 16, 32, 64, 128, 256 that holds it, for any D that
// is a multiple of 4 (rows then stay 16-byte aligned; dims past D are the tree's zero padding) -- or 0: generic layout.
uint32_t subwave_width(const f2v_ctx *c) {
    if (!c->use_quarter || c->D % 4u != 0u || c->D > 256u) return 0u;
    uint32_t w = 16;
    while (w < c->D) w <<= 1;
    return w;
}

// The sub-wave layouts: an item's row lies in LPI lanes of NB dwordx4 each, U neighbour rows are in flight per item, and a
// wavefront holds `per_wave` items.  Everything that depends on a layout -- the planners' items per workgroup, the kernel
// instantiations a launch chooses from (dispatch_subwave) -- reads this table.
struct SubwaveLayout {
    uint32_t width;
    int lpi, nb, u;
    uint32_t per_wave;
};
constexpr SubwaveLayout kSubwave[] = {{16, 4, 1, 8, 16}, {32, 8, 1, 8, 8}, {64, 16, 1, 8, 4}, {128, 16, 2, 4, 4}, {256, 16, 4, 4, 4}};

// items per wavefront on the layout of this width (0: the generic layout, one item per wavefront)
constexpr uint32_t items_per_wave(uint32_t width) {
    for (const SubwaveLayout &l : kSubwave)
        if (l.width == width) return l.per_wave;
    return 1u;
}

// items one workgroup of the step kernel covers, and tree nodes one workgroup covers (= its wavefronts)
uint32_t items_per_block(const f2v_ctx *c) { return items_per_wave(subwave_width(c)) * (uint32_t)c->waves_per_block; }

template <int V> using Int = std::integral_constant<int, V>;

// f(OPT, LPI, NB, U, FULL) on layout I of the table with U rows in flight
template <int I, int U, typename F>
int subwave_case(int math, bool full, F &f) {
    auto run = [&](auto O) {
        if (full) f(O, Int<kSubwave[I].lpi>{}, Int<kSubwave[I].nb>{}, Int<U>{}, std::true_type{});
        else f(O, Int<kSubwave[I].lpi>{}, Int<kSubwave[I].nb>{}, Int<U>{}, std::false_type{});
    };
    if (math == 5) run(Int<5>{});
    else run(Int<6>{});
    return F2V_OK;
}

// Call f(OPT, LPI, NB, U, FULL) -- std::integral_constants -- for the sub-wave kernel that runs `math` on the layout `width`.
// OPT: 5 or 6 (math 7 runs 6); FULL: the rows fill the layout (D == width).  The launch forms do not instantiate the same
// kernels, and f is only instantiated for what its form runs: NARROWEST is the form's narrowest layout, U8_AT_128 says whether
// "rows_in_flight" = 8 selects U = 8 at width 128 (elsewhere U is the table's).
template <uint32_t NARROWEST, bool U8_AT_128, typename F>
int dispatch_subwave(const f2v_ctx *c, int math, uint32_t width, F &&f) {
    static_assert(NARROWEST == kSubwave[0].width || NARROWEST == kSubwave[1].width, "a form may leave out the narrowest layout only");
    const bool full = width == c->D;
    switch (width) {
        case kSubwave[0].width:
            if constexpr (NARROWEST <= kSubwave[0].width) return subwave_case<0, kSubwave[0].u>(math, full, f);
            break;
        case kSubwave[1].width: return subwave_case<1, kSubwave[1].u>(math, full, f);
        case kSubwave[2].width: return subwave_case<2, kSubwave[2].u>(math, full, f);
        case kSubwave[3].width:
            if constexpr (U8_AT_128)
                if (c->rows_in_flight == 8) return subwave_case<3, 8>(math, full, f);
            return subwave_case<3, kSubwave[3].u>(math, full, f);
        case kSubwave[4].width: return subwave_case<4, kSubwave[4].u>(math, full, f);
    }
    return fail(F2V_ESTATE, "no sub-wave kernel of this launch form runs rows of width %u", width);
}

// Where a split row (degree > chunk) is cut into pieces: after every `chunk` neighbours, and -- "class_cut", the default --
// also wherever the (ascending) neighbour ids cross from one eighth of the id range into the next, so that all neighbours of
// a piece belong to ONE of the kIdClasses id ranges and the piece can run on the XCD whose L2 caches that range
// ("piece_affinity").  The cuts are part of the summation order (a piece accumulates from zero, the pieces' sums are combined
// in order): the oracle restates exactly this rule (oracle/f2v_oracle.c: piece_cuts), and it depends on nothing but the
// row's neighbour ids, the chunk and N -- not on the machine, the placement or the number of GPUs.
// Appends the offsets of the pieces' first neighbours and, last, the degree.
constexpr uint32_t kIdClasses = 8;
void piece_cuts(const f2v_ctx *c, uint32_t row, std::vector<uint32_t> &cuts) {
    const uint32_t rp = c->rowptr[row], deg = c->rowptr[row + 1] - rp;
    if (!c->class_cut) {
        for (uint32_t b = 0; b < deg; b += c->chunk) cuts.push_back(b);
        cuts.push_back(deg);
        return;
    }
    auto cls_of = [&](uint32_t e) { return (uint32_t)(((uint64_t)c->colids[rp + e] * kIdClasses) / c->n); };
    uint32_t start = 0, cls = cls_of(0);
    cuts.push_back(0);
    for (uint32_t e = 1; e < deg; e++) {
        const uint32_t ce = cls_of(e);
        if (ce != cls || e - start == c->chunk) {
            cuts.push_back(e);
            start = e;
            cls = ce;
        }
    }
    cuts.push_back(deg);
}

// Is row i cut into pieces?  More than `chunk` neighbours.  (Round 3 tried cutting rows of 17 ... 128 neighbours at the id-class
// boundaries as well, so that their pieces get "piece_affinity" too: L2 hit rate 0.513 -> 0.537, +8 ... 11 % time for the extra
// partial sums -- profiles/r03_class_split_min_rejected.txt.)
bool is_split(const f2v_ctx *c, uint32_t i) { return c->chunk != 0 && c->rowptr[i + 1] - c->rowptr[i] > c->chunk; }

// Compulsory bytes of one minibatch: every DISTINCT embedding row it reads (its own rows and their neighbours) once, every
// row it writes once, its neighbour ids and work items once -- what would still cross HBM if everything read twice inside
// the minibatch came from a cache the second time.  (The ns sampled rows, the partial sums of split rows and rowptr are
// left out: a lower bound.)
uint64_t compulsory_bytes(const f2v_ctx *c, SeenScratch &sc, uint32_t row_lo, uint32_t row_hi, bool walk, uint64_t nnz, uint64_t n_items) {
    if (sc.seen.size() != c->n) { sc.seen.assign(c->n, 0u); sc.stamp = 0; }
    if (++sc.stamp == 0) { std::fill(sc.seen.begin(), sc.seen.end(), 0u); sc.stamp = 1; }
    const uint32_t st = sc.stamp;
    uint32_t *seen = sc.seen.data();
    uint64_t distinct = 0;
    const uint32_t *ids = walk ? nullptr : c->colids.data();
    for (uint32_t i = row_lo; i < row_hi; i++) {
        if (seen[i] != st) { seen[i] = st; distinct++; }
        if (!ids) continue;  // walk samples change every epoch: only the rows themselves are counted
        for (uint32_t k = c->rowptr[i]; k < c->rowptr[i + 1]; k++) {
            const uint32_t j = ids[k];
            if (seen[j] != st) { seen[j] = st; distinct++; }
        }
    }
    return distinct * 4ull * c->D + (uint64_t)(row_hi - row_lo) * 4ull * c->D + nnz * 4ull + n_items * sizeof(Item);
}

// The plan cache may hold a few epochs' worth of items (one epoch: every row or piece once -- about nnz / chunk + 8 per split
// row + n); beyond that it is dropped and rebuilt on demand (a run that alternates batch sizes).
size_t plan_cache_limit(const f2v_ctx *c) {
    const size_t epoch = (size_t)(c->nnz / std::max<uint32_t>(c->chunk, 1u)) + 2 * (size_t)c->n + 1024;
    return std::max<size_t>(8 * ((size_t)c->n + 1024), 3 * epoch);
}

// Work items of one launch (rows [row_lo,row_hi), CSR neighbours or walk samples): a whole row, or
// `chunk`-neighbour pieces of a hub row, longest first (the longest waves start first and the four quarters of a
// wave get items of nearly equal length).  Host-side, cached per launch shape.
//
// Who may wait for whom.  Tree nodes WAIT for the partial sums they add (one launch per minibatch), so what they wait
// for must be running or done whatever else the GPU is doing.  Workgroups go to the 8 XCDs round robin (workgroup b
// to XCD b mod 8) and every XCD starts its workgroups in index order; inside one process that is enough.  But a
// second process whose own waiting nodes fill one XCD can keep this launch's first workgroups from starting there
// while the other seven XCDs run ahead into the tree nodes -- two such processes can wait for each other (seen with
// three replays sharing one card: bounded by the time-out, but seconds long).  So the bulk of the waiting -- the
// lowest tree level, one node per group of `fanin` pieces -- is tied to an XCD: a group gets a CLASS 0..7 and its
// pieces and its node are placed in workgroups whose index is congruent to the class modulo 8 (whole rows and, at
// the very end, inert padding items fill the gaps): such a node only ever waits for workgroups of its OWN XCD with
// a smaller index, which that XCD has started before it.  The upper levels are 1/fanin as many nodes -- too few to
// fill an XCD, so they cannot take part in such a ring -- and stay unconstrained.
const Plan &plan_for(f2v_ctx *c, uint32_t row_lo, uint32_t row_hi, bool walk) {
    const auto key = std::make_tuple(row_lo, row_hi, walk ? 1 : 0);
    auto itp = c->plans.find(key);
    if (itp != c->plans.end()) return itp->second;
    if (c->plan_items.h.size() > plan_cache_limit(c)) drop_plans(c);  // bound the cache
    constexpr uint32_t kXcds = 8;
    const uint32_t ipb = items_per_block(c), npb = (uint32_t)c->waves_per_block;
    Plan p;
    p.item_off = c->plan_items.h.size();
    std::vector<Item> whole;  // rows that stay one item
    whole.reserve(row_hi - row_lo);
    struct Node { uint32_t row, in_slot, n, cut; };  // cut: index of the row's first piece boundary in `cuts`
    std::vector<Node> cur, nxt;
    std::vector<uint32_t> cuts;  // per split row: offsets of its pieces' first neighbours, then its degree
    uint32_t slots = 0;
    for (uint32_t i = row_lo; i < row_hi; i++) {
        if (walk) {
            whole.push_back(Item{i, i * (uint32_t)kWalkLength, (uint32_t)kWalkLength, kItemFirst | kItemLast});
            p.nnz += kWalkLength;
            continue;
        }
        const uint32_t rp = c->rowptr[i], deg = c->rowptr[i + 1] - rp;
        p.nnz += deg;
        if (is_split(c, i)) {
            const uint32_t cut0 = (uint32_t)cuts.size();
            piece_cuts(c, i, cuts);
            const uint32_t nc = (uint32_t)cuts.size() - cut0 - 1;
            cur.push_back(Node{i, slots, nc, cut0});
            slots += nc;
        } else {
            whole.push_back(Item{i, rp, deg, kItemFirst | kItemLast});
        }
    }
    p.n_hubs = (uint32_t)cur.size();
    p.n_chunks = slots;
    std::vector<Item> items;
    items.reserve(whole.size() + slots + 64);
    // inert filler: an empty piece of row `row_lo` whose (zero) partial sum goes to a slot of its own that no node reads --
    // the kernels need no special case for it
    Item pad_item{row_lo, 0, 0, kItemPartial};
    bool padded = false;
    const FinItem pad_node{0, 0, kFinToStage, 0};
    std::stable_sort(whole.begin(), whole.end(), [](const Item &x, const Item &y) { return x.cnt > y.cnt; });
    if (!cur.empty()) {
        // Lowest tree level first: one node per GROUP of `fanin` consecutive pieces of a hub.  A group -- its pieces and
        // its node -- gets the class that has been given the fewest neighbours so far (a giant hub thus spreads over all XCDs).
        std::vector<Item> queue[kXcds];
        std::vector<FinItem> nq[kXcds];
        uint64_t load[kXcds] = {}, aload[kXcds] = {};  // neighbours given to every class so far: a group goes to the lightest one
        for (const Node &nd : cur) {
            const uint32_t rp = c->rowptr[nd.row];
            const uint32_t *cut = cuts.data() + nd.cut;
            const uint32_t G = c->fanin < 2 ? nd.n : c->fanin;
            const uint32_t nout = (nd.n + G - 1) / G;
            for (uint32_t o = 0; o < nout; o++) {
                const uint32_t k0 = o * G, k1 = std::min(nd.n, k0 + G);
                uint32_t cls = 0;
                for (uint32_t k = 1; k < kXcds; k++)
                    if (load[k] < load[cls]) cls = k;
                load[cls] += cut[k1] - cut[k0];
                for (uint32_t k = k0; k < k1; k++) {
                    const uint32_t b = cut[k], e = cut[k + 1];
                    // "piece_affinity" (DESIGN.md section 3): a piece goes to the XCD that owns the id range of its (ascending)
                    // neighbours -- the lightest of the XCDs whose ranges it touches: midpoints alone leave the outer ranges short
                    // of work and cost 40 % -- so that every L2 caches an eighth of the matrix instead of all eight the same
                    // hubs: RMAT-20, batch 65536: L2 hit rate 0.31 -> 0.42, L2-miss reads -17 %, epoch time -7...-10 %.
                    // Placement only: bits do not change.  The group's node stays in class `cls`, so it may now wait for other
                    // XCDs' workgroups: fine inside one process (index order), not with a second process on the card that could
                    // fill an XCD with ITS waiting nodes -- ranks that share a card are detected (f2v_push_attach) and keep
                    // the same-XCD groups.
                    uint32_t pc = cls;
                    if (c->piece_affinity && !c->shared_card) {
                        const uint32_t c0 = (uint32_t)(((uint64_t)c->colids[rp + b] * kXcds) / c->n), c1 = (uint32_t)(((uint64_t)c->colids[rp + e - 1] * kXcds) / c->n);
                        pc = c0;
                        for (uint32_t q = c0 + 1; q <= c1; q++)
                            if (aload[q] < aload[pc]) pc = q;
                        aload[pc] += e - b;
                    }
                    queue[pc].push_back(Item{nd.row, rp + b, e - b, kItemPartial | (k == 0 ? kItemFirst : 0u) | (k == nd.n - 1 ? kItemLast : 0u) | (nd.in_slot + k)});
                }
                nq[cls].push_back(FinItem{nd.in_slot + k0, k1 - k0, nout == 1 ? kFinToStage : slots + o, nd.row});
            }
            if (nout > 1) {
                nxt.push_back(Node{nd.row, slots, nout, 0});
                slots += nout;
            }
        }
        for (auto &q : queue) std::stable_sort(q.begin(), q.end(), [](const Item &x, const Item &y) { return x.cnt > y.cnt; });
        // One workgroup per class per round, longest first overall: a class's workgroup takes its own pieces as long as
        // they are at least as long as the longest whole row still waiting (whole rows may run anywhere), else whole rows.
        size_t pos[kXcds] = {}, wpos = 0;
        {
            for (bool more = true; more;) {
                more = false;
                for (uint32_t k = 0; k < kXcds; k++) {
                    for (uint32_t j = 0; j < ipb; j++) {
                        const bool mine = pos[k] < queue[k].size(), any = wpos < whole.size();
                        if (mine && (!any || queue[k][pos[k]].cnt >= whole[wpos].cnt)) items.push_back(queue[k][pos[k]++]);
                        else if (any) items.push_back(whole[wpos++]);
                        else { items.push_back(pad_item); padded = true; }
                    }
                    more = more || pos[k] < queue[k].size();
                }
            }
        }
        items.insert(items.end(), whole.begin() + wpos, whole.end());
        // the nodes' workgroups follow the items': their first one must again be a multiple of 8
        while (items.size() % ((size_t)kXcds * ipb) != 0) { items.push_back(pad_item); padded = true; }
        p.fin_off[0] = c->plan_hubs.h.size();
        size_t npos[kXcds] = {};
        for (bool more = true; more;) {
            more = false;
            for (uint32_t k = 0; k < kXcds; k++) {
                for (uint32_t j = 0; j < npb; j++) c->plan_hubs.h.push_back(npos[k] < nq[k].size() ? nq[k][npos[k]++] : pad_node);
                more = more || npos[k] < nq[k].size();
            }
        }
        p.fin_cnt[0] = (uint32_t)(c->plan_hubs.h.size() - p.fin_off[0]);
        p.n_levels = 1;
        cur.swap(nxt);
    } else {
        items.insert(items.end(), whole.begin(), whole.end());
    }
    const size_t items_at = c->plan_items.h.size();
    c->plan_items.h.insert(c->plan_items.h.end(), items.begin(), items.end());
    p.n_items = (uint32_t)items.size();
    // upper levels: groups of `fanin` sums are added in order until one is left.  Their nodes are few (1/fanin of the
    // level below): wherever they wait, they cannot fill an XCD, so they are packed without regard to classes.
    while (!cur.empty() && p.n_levels < kMaxFinLevels) {
        p.fin_off[p.n_levels] = c->plan_hubs.h.size();
        nxt.clear();
        for (const Node &nd : cur) {
            const uint32_t G = (p.n_levels == kMaxFinLevels - 1 || c->fanin < 2) ? nd.n : c->fanin;
            const uint32_t nout = (nd.n + G - 1) / G;
            if (nout == 1) {
                c->plan_hubs.h.push_back(FinItem{nd.in_slot, nd.n, kFinToStage, nd.row});
            } else {
                for (uint32_t o = 0; o < nout; o++)
                    c->plan_hubs.h.push_back(FinItem{nd.in_slot + o * G, std::min(G, nd.n - o * G), slots + o, nd.row});
                nxt.push_back(Node{nd.row, slots, nout, 0});
                slots += nout;
            }
        }
        p.fin_cnt[p.n_levels] = (uint32_t)(c->plan_hubs.h.size() - p.fin_off[p.n_levels]);
        p.n_levels++;
        cur.swap(nxt);
    }
    if (padded) {  // the fillers' slot: one past every slot a node reads
        for (size_t k = items_at; k < items_at + p.n_items; k++)
            if (c->plan_items.h[k].cnt == 0 && c->plan_items.h[k].flags == kItemPartial) c->plan_items.h[k].flags = kItemPartial | slots;
        slots++;
    }
    p.n_slots = slots;
    if (slots > kItemSlotMask) c->plan_overflow = true;  // the slot index would run into the item's flag bits: the caller fails the call
    if (c->count_compulsory) p.compulsory = compulsory_bytes(c, c->seen_scratch, row_lo, row_hi, walk, p.nnz, p.n_items);
    c->max_slots = std::max<size_t>(c->max_slots, slots);
    return c->plans.emplace(key, p).first->second;
}

// Minibatches per chained launch ("chain_rows" rows per launch, at most 4096 minibatches)
uint32_t chain_len(const f2v_ctx *c, uint32_t batch, bool wide_form = false) {
    uint64_t k = (uint64_t)(wide_form ? c->wide_rows : c->chain_rows) / std::max(batch, 1u);
    // handed-on rows are read through a buffer resource that starts at the launch's first row, at 32-bit byte offsets (load16_agent)
    k = std::min<uint64_t>(k, 0xFFFFFFFFull / ((uint64_t)std::max(batch, 1u) * c->D * sizeof(float)));
    return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(k, 1));
}

// The sub-wave layout the wide form runs a D on.  Narrow rows on a wider layout leave part of every lane group idle, but a
// wavefront then holds fewer items -- and a wavefront of a chained launch is as late as the latest of its items.  Measured
// (tools/wide_min_width.py, tools/cora_configs.py): cora at D = 16, 1200 epochs: 0.098 s on the 16-wide layout (16 items per
// wavefront), 0.086 s on 32, 0.0795 s on 64 (4 items); RMAT-20 at D = 16: 32 wide is 10 % faster than 16 at batch 256 and 17 %
// slower at 2048, 64 wide slower everywhere (throughput counts there).  "wide_min_width" = 0 chooses: 64 for small graphs (up to
// 2 M nonzeros), 32 for minibatches of up to 1024 rows, else the narrowest layout that holds D.  The zero padding of the wider
// tree changes no bit.
uint32_t wide_width(const f2v_ctx *c, uint32_t batch) {
    const uint32_t floor_w = c->wide_min_width ? c->wide_min_width : (c->nnz <= (2ull << 20) ? 64u : batch <= 1024u ? 32u : 16u);
    return std::max(subwave_width(c), floor_w);
}
uint32_t wide_items_per_block(uint32_t width) { return 4u * items_per_wave(width); }

// the wide form of a chained launch: jobs add at most 32 LDS slots, so the fan-in groups must fit
bool wide_usable(const f2v_ctx *c) { return c->wide && c->fanin >= 2 && c->fanin <= 32 && c->waves_per_block == 4; }

bool chain_usable(const f2v_ctx *c, int math, uint32_t batch, int bs_mode, bool sharded) {
    const uint32_t nb = (uint32_t)(((uint64_t)c->n + batch - 1) / batch);
    (void)bs_mode;  // -bs 1 chains too: its per-row sample windows are gathered per item, and those gathers wait for rows like any other
    (void)math;     // option 7 chains too: its five walk samples per row are gathered (and waited for) like CSR neighbours
    // rows narrower than a 128-byte line (D = 16, 8, 4 ...): only in the wide form, whose handed-off rows are read with agent-scope
    // loads alone, and only where no line holds rows of two minibatches (every reader then treats all of a line's rows alike)
    const bool lines_ok = c->D % 32u == 0u || (wide_usable(c) && batch <= c->wide_max_batch && (chain_len(c, batch, true) >= 2 || c->wide_single) && ((uint64_t)batch * c->D) % 32u == 0u);
    return c->chain && !sharded && c->merge_fin && c->xcc_round_robin && !c->capturing && !c->use_graph &&
           subwave_width(c) != 0 && lines_ok && batch <= c->chain_max_batch && nb >= 2 && (chain_len(c, batch) >= 2 || c->wide_single);
}

// The work of minibatches [b0, b0+K) of batch size `batch` as ONE launch: per minibatch its items (rows whose neighbours all
// lie outside the launch's earlier minibatches first: their workgroups never wait), then its combine-tree nodes; a
// descriptor per workgroup with the minibatches it has to wait for.  Same pieces, same fan-in, same slots-in-chunk-order as
// plan_for: the summation order -- and with it every bit of the result -- does not depend on how minibatches are launched.
const ChainPlan &chain_plan_for(f2v_ctx *c, uint32_t b0, uint32_t K, uint32_t batch, bool walk) {
    const auto key = std::make_tuple(b0, K, batch, walk ? 1 : 0);
    auto itp = c->chains.find(key);
    if (itp != c->chains.end()) return itp->second;
    if (c->plan_items.h.size() > plan_cache_limit(c)) drop_plans(c);  // bound the cache
    const uint32_t ipb = items_per_block(c), npb = (uint32_t)c->waves_per_block;
    ChainPlan p;
    p.first_batch = b0;
    p.n_batches = K;
    p.item_off = c->plan_items.h.size();
    p.fin_off = c->plan_hubs.h.size();
    p.wg_off = c->plan_wg.h.size();
    p.lo = (uint32_t)std::min<uint64_t>((uint64_t)b0 * batch, c->n);
    uint32_t slots = 0;
    struct DI { Item it; uint64_t dep; };
    std::vector<DI> items;
    struct Node { uint32_t row, in_slot, n; };
    std::vector<Node> cur, nxt;
    std::vector<uint32_t> cutbuf;
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t lo = (uint32_t)std::min<uint64_t>((uint64_t)(b0 + k) * batch, c->n);
        const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + batch, c->n);
        p.hi = hi;
        items.clear();
        cur.clear();
        uint64_t nnz = 0;
        auto dep_of = [&](uint32_t from, uint32_t to) -> uint64_t {  // 1 + the LAST row of this launch's earlier minibatches among the neighbours [from,to): 0 = independent
            uint64_t m = 0;
            for (uint32_t e = from; e < to; e++) {
                const uint32_t j = c->colids[e];
                if (j >= p.lo && j < lo) m = std::max<uint64_t>(m, (uint64_t)(j - p.lo) + 1);
            }
            return m;
        };
        for (uint32_t i = lo; i < hi; i++) {
            if (walk) {  // option 7: the row's five walk samples of the epoch (they change every epoch: no ordering hint)
                items.push_back(DI{Item{i, i * (uint32_t)kWalkLength, (uint32_t)kWalkLength, kItemFirst | kItemLast}, 0});
                nnz += kWalkLength;
                continue;
            }
            const uint32_t rp = c->rowptr[i], deg = c->rowptr[i + 1] - rp;
            nnz += deg;
            if (is_split(c, i)) {
                cutbuf.clear();
                piece_cuts(c, i, cutbuf);
                const uint32_t nc = (uint32_t)cutbuf.size() - 1;
                for (uint32_t q = 0; q < nc; q++) {
                    const uint32_t b = cutbuf[q], e = cutbuf[q + 1];
                    items.push_back(DI{Item{i, rp + b, e - b, kItemPartial | (q == 0 ? kItemFirst : 0u) | (q == nc - 1 ? kItemLast : 0u) | (slots + q)}, dep_of(rp + b, rp + e)});
                }
                cur.push_back(Node{i, slots, nc});
                slots += nc;
                p.n_hubs++;
                p.n_chunks += nc;
            } else {
                items.push_back(DI{Item{i, rp, deg, kItemFirst | kItemLast}, dep_of(rp, rp + deg)});
            }
        }
        // independent items first (longest first), then the dependent ones, those that wait for the oldest rows first
        std::stable_sort(items.begin(), items.end(), [](const DI &x, const DI &y) {
            if ((x.dep != 0) != (y.dep != 0)) return x.dep == 0;
            if (x.dep != y.dep && x.dep != 0) return x.dep < y.dep;
            return x.it.cnt > y.it.cnt;
        });
        if (items.size() % ipb != 0) {  // inert fillers: empty pieces whose (zero) sum goes to a slot no node reads
            const Item pad{lo, 0, 0, kItemPartial | slots};
            slots++;
            while (items.size() % ipb != 0) items.push_back(DI{pad, 0});
        }
        WgDesc bd{};
        bd.lo = lo;
        p.last_lo = lo;
        bd.item_off = (uint32_t)(c->plan_items.h.size() - p.item_off);
        bd.n_items = (uint32_t)items.size();
        bd.step_blocks = bd.n_items / ipb;
        bd.fin_off = (uint32_t)(c->plan_hubs.h.size() - p.fin_off);
        bd.index = b0 + k;
        const size_t wg_at = c->plan_wg.h.size();  // (fin_n is known only below: the descriptors are patched then)
        for (uint32_t w = 0; w < bd.step_blocks; w++) { bd.blk = w; c->plan_wg.h.push_back(bd); }
        for (const DI &d : items) c->plan_items.h.push_back(d.it);
        // the combine trees of this minibatch's split rows, level by level (fan-in groups in chunk order, as plan_for)
        uint32_t fin_n = 0;
        for (int level = 0; !cur.empty(); level++) {
            nxt.clear();
            for (const Node &nd : cur) {
                const uint32_t G = (level == kMaxFinLevels - 1 || c->fanin < 2) ? nd.n : c->fanin;
                const uint32_t nout = (nd.n + G - 1) / G;
                if (nout == 1) {
                    c->plan_hubs.h.push_back(FinItem{nd.in_slot, nd.n, kFinToStage, nd.row});
                    fin_n++;
                } else {
                    for (uint32_t o = 0; o < nout; o++) {
                        c->plan_hubs.h.push_back(FinItem{nd.in_slot + o * G, std::min(G, nd.n - o * G), slots + o, nd.row});
                        fin_n++;
                    }
                    nxt.push_back(Node{nd.row, slots, nout});
                    slots += nout;
                }
            }
            cur.swap(nxt);
        }
        while (fin_n % npb != 0) { c->plan_hubs.h.push_back(FinItem{0, 0, kFinToStage, 0}); fin_n++; }
        bd.fin_n = fin_n;
        const uint32_t node_blocks = fin_n / npb;
        // (the nodes must directly follow their minibatch's items: later minibatches' items wait for the rows the roots write,
        // and a waiter may only ever wait for a SMALLER workgroup index -- letting the nodes trail by a few minibatches, so that
        // they poll less, was tried: it buys 3-9 % without the row waits and deadlocks with them, caught by the bounded waits)
        for (uint32_t w = 0; w < node_blocks; w++) { bd.blk = bd.step_blocks + w; c->plan_wg.h.push_back(bd); }
        for (size_t w = wg_at; w < c->plan_wg.h.size(); w++) c->plan_wg.h[w].fin_n = fin_n;
        p.n_wgs += bd.step_blocks + node_blocks;
        p.n_fin += fin_n;
        p.nnz += nnz;
        if (c->count_compulsory) p.compulsory += compulsory_bytes(c, c->seen_scratch, lo, hi, walk, nnz, bd.n_items);
    }
    p.n_slots = slots;
    if (slots > kItemSlotMask) c->plan_overflow = true;
    c->max_slots = std::max<size_t>(c->max_slots, slots);
    return c->chains.emplace(key, p).first->second;
}


// Minibatches [b0, b0+K) as ONE launch of qwide_chain_kernel: per minibatch the helper workgroups of its multi-group rows,
// then their finishers, then the workgroups that pack whole low-degree rows and rows of one fan-in group, then the
// combine-tree nodes above the units of rows with more than fanin^2 pieces.  Pieces (piece_cuts), fan-in groups and the
// order of every addition are those of plan_for / chain_plan_for: the result does not depend on which form ran.
// (built into vectors of its own, offsets relative to them: the plans of an epoch are independent of each other and are built by
// several host threads, wide_plans_for_epoch -- one thread took 0.33 s for RMAT-20 at batch 256 and, by the same count, ~5 s for RMAT-24)
struct WideParts {
    std::vector<Item> items;
    std::vector<WJob> jobs;
    std::vector<WideDesc> wide;
    std::vector<FinItem> hubs;
};
WidePlan build_wide_plan(const f2v_ctx *c, uint32_t b0, uint32_t K, uint32_t batch, bool walk, WideParts &out, SeenScratch &seen) {
    const uint32_t layout = wide_width(c, batch);
    const uint32_t ipb = wide_items_per_block(layout);        // lane groups per workgroup = items per round
    const uint32_t pslots = std::max<uint32_t>(ipb, 32u);      // piece slots of a phase (PSLOTS of the kernel)
    const uint32_t F = c->fanin;
    WidePlan p;
    p.width = layout;
    p.first_batch = b0;
    p.n_batches = K;
    p.item_off = p.fin_off = p.wg_off = p.job_off = 0;  // (relative to `out`; wide_plan_append moves them)
    p.lo = (uint32_t)std::min<uint64_t>((uint64_t)b0 * batch, c->n);
    uint32_t slots = 0;  // partial sums in HBM: helpers' group sums, units' sums, upper tree levels

    struct Prog {  // one workgroup: items laid out round by round (ipb per round), jobs in execution order
        std::vector<Item> items;
        std::vector<WJob> jobs;
        uint32_t phases = 0;
    };
    struct Piece { Item it; uint64_t dep; };
    struct Group { uint32_t first, n; uint64_t dep; };  // pieces [first, first+n) of `pieces`
    struct Pack { uint32_t first, n; uint64_t dep; uint8_t kind; uint32_t dst, row; };  // a whole row (n = 1, direct) or a one-group unit
    std::vector<Piece> pieces;
    std::vector<Pack> packs;
    std::vector<Prog> helpers, finishers, packed;
    std::vector<uint32_t> cutbuf;
    struct Node { uint32_t row, in_slot, n; };
    std::vector<Node> cur, nxt;

    // One phase's items: every item has been given its LDS slot (= the order in which the jobs add) when it was appended; they
    // RUN in the order of what they wait for -- independent ones first, the ones that read the most recently written rows in
    // the last round -- padded to whole rounds; the last round carries kItemPhaseEnd.
    auto close_phase = [&](Prog &g, std::vector<Piece> &ph, uint32_t lo_row) {
        if (ph.empty()) return;
        std::stable_sort(ph.begin(), ph.end(), [](const Piece &x, const Piece &y) { return x.dep < y.dep; });
        const size_t at = g.items.size();
        for (const Piece &pc : ph) g.items.push_back(pc.it);
        while ((g.items.size() - at) % ipb != 0) g.items.push_back(Item{lo_row, 0, 0, kItemIdle});
        for (size_t k = g.items.size() - ipb; k < g.items.size(); k++) g.items[k].flags |= kItemPhaseEnd;
        g.phases++;
        ph.clear();
    };
    auto slotted = [](Piece pc, size_t slot) { pc.it.flags |= (uint32_t)slot; return pc; };
    auto mkjob = [](size_t src, uint32_t n, uint8_t kind, size_t phase, uint32_t dst, uint32_t row) {
        WJob j{};
        j.src = (uint8_t)src; j.n = (uint8_t)n; j.kind = kind; j.phase = (uint8_t)phase; j.dst = dst; j.row = row;
        return j;
    };
    // the jobs of one phase as passes of up to 8
    auto add_pass = [&](Prog &g, std::vector<WJob> &js) {
        for (size_t k = 0; k < js.size(); k += 8) {
            const uint8_t len = (uint8_t)std::min<size_t>(8, js.size() - k);
            for (size_t u = 0; u < len; u++) { js[k + u].pass_len = len; g.jobs.push_back(js[k + u]); }
        }
        js.clear();
    };

    for (uint32_t k = 0; k < K; k++) {
        const uint32_t lo = (uint32_t)std::min<uint64_t>((uint64_t)(b0 + k) * batch, c->n);
        const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + batch, c->n);
        p.hi = hi;
        p.last_lo = lo;
        pieces.clear(); packs.clear(); helpers.clear(); finishers.clear(); packed.clear(); cur.clear();
        uint64_t nnz = 0;
        uint32_t mb_items = 0;
        auto dep_of = [&](uint32_t from, uint32_t to) -> uint64_t {  // 1 + the LAST row of this launch's earlier minibatches among the neighbours [from,to): 0 = independent
            uint64_t m = 0;
            for (uint32_t e = from; e < to; e++) {
                const uint32_t j = c->colids[e];
                if (j >= p.lo && j < lo) m = std::max<uint64_t>(m, (uint64_t)(j - p.lo) + 1);
            }
            return m;
        };
        for (uint32_t i = lo; i < hi; i++) {
            if (walk) {  // option 7: the row's five walk samples of the epoch
                pieces.push_back(Piece{Item{i, i * (uint32_t)kWalkLength, (uint32_t)kWalkLength, kItemFirst | kItemLast | kItemDirect}, 0});
                packs.push_back(Pack{(uint32_t)pieces.size() - 1, 1, 0, kJobRow, 0, i});
                nnz += kWalkLength;
                continue;
            }
            const uint32_t rp = c->rowptr[i], deg = c->rowptr[i + 1] - rp;
            nnz += deg;
            if (!is_split(c, i)) {
                pieces.push_back(Piece{Item{i, rp, deg, kItemFirst | kItemLast | kItemDirect}, dep_of(rp, rp + deg)});
                packs.push_back(Pack{(uint32_t)pieces.size() - 1, 1, pieces.back().dep, kJobRow, 0, i});
                continue;
            }
            cutbuf.clear();
            piece_cuts(c, i, cutbuf);
            const uint32_t P = (uint32_t)cutbuf.size() - 1;
            p.n_hubs++;
            p.n_chunks += P;
            const uint32_t first_piece = (uint32_t)pieces.size();
            for (uint32_t q = 0; q < P; q++) {
                const uint32_t b = cutbuf[q], e = cutbuf[q + 1];
                pieces.push_back(Piece{Item{i, rp + b, e - b, (q == 0 ? kItemFirst : 0u) | (q == P - 1 ? kItemLast : 0u)}, dep_of(rp + b, rp + e)});
            }
            // units of F*F pieces (F groups of F): one unit is the whole row unless the row has more pieces than that
            const uint32_t per_unit = F * F;
            const uint32_t n_units = (P + per_unit - 1) / per_unit;
            uint32_t unit_base = 0;
            if (n_units > 1) {
                unit_base = slots;
                slots += n_units;
                cur.push_back(Node{i, unit_base, n_units});
            }
            for (uint32_t u = 0; u < n_units; u++) {
                const uint32_t u0 = u * per_unit, u1 = std::min(P, u0 + per_unit);
                const uint8_t out_kind = n_units > 1 ? kJobPart : kJobRow;
                const uint32_t out_dst = n_units > 1 ? unit_base + u : 0u;
                const uint32_t G = (u1 - u0 + F - 1) / F;
                if (G == 1) {  // one fan-in group: packed with other small rows
                    uint64_t dep = 0;
                    for (uint32_t q = u0; q < u1; q++) dep = std::max(dep, pieces[first_piece + q].dep);
                    packs.push_back(Pack{first_piece + u0, u1 - u0, dep, out_kind, out_dst, i});
                    continue;
                }
                std::vector<Group> groups(G);
                for (uint32_t g = 0; g < G; g++) {
                    const uint32_t q0 = u0 + g * F, q1 = std::min(u1, q0 + F);
                    uint64_t dep = 0;
                    for (uint32_t q = q0; q < q1; q++) dep = std::max(dep, pieces[first_piece + q].dep);
                    groups[g] = Group{first_piece + q0, q1 - q0, dep};
                }
                // the finisher keeps the groups that depend on the most recently written rows (they wait longest)
                std::vector<uint32_t> order(G);
                for (uint32_t g = 0; g < G; g++) order[g] = g;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return groups[x].dep < groups[y].dep; });
                const uint32_t n_own = std::min(G, std::max(1u, c->wide_finish));
                std::vector<uint32_t> own(order.end() - n_own, order.end());   // oldest dependency first, the latest last
                std::vector<uint32_t> rest(order.begin(), order.end() - n_own);
                std::sort(rest.begin(), rest.end());
                const uint32_t l0_base = slots;
                if (!rest.empty()) slots += G;
                // helpers: `wide_span` groups each, group sums written through to HBM
                for (size_t h0 = 0; h0 < rest.size(); h0 += std::max(1u, c->wide_span)) {
                    Prog g;
                    std::vector<Piece> ph;
                    std::vector<WJob> js;
                    for (size_t h = h0; h < std::min(rest.size(), h0 + std::max(1u, c->wide_span)); h++) {
                        const Group &gr = groups[rest[h]];
                        if (ph.size() + gr.n > pslots) { close_phase(g, ph, lo); add_pass(g, js); }
                        js.push_back(mkjob(ph.size(), gr.n, kJobPart, g.phases, l0_base + rest[h], i));
                        for (uint32_t q = 0; q < gr.n; q++) ph.push_back(slotted(pieces[gr.first + q], ph.size()));
                    }
                    close_phase(g, ph, lo);
                    add_pass(g, js);
                    helpers.push_back(std::move(g));
                }
                // finisher: its own groups (sums -> LDS), the helpers' sums imported before its last phase, then the unit's sum
                {
                    Prog g;
                    std::vector<Piece> ph;
                    std::vector<WJob> js, imports;
                    for (uint32_t r : rest) imports.push_back(mkjob(0, 0, kJobImport, 0, pslots + r, l0_base + r));
                    // phases of the own groups, in `own` order; the last phase starts with the last group that does not fit the one before
                    std::vector<std::vector<uint32_t>> phases(1);
                    {
                        uint32_t used = 0;
                        for (uint32_t g2 : own) {
                            if (used + groups[g2].n > pslots) { phases.emplace_back(); used = 0; }
                            phases.back().push_back(g2);
                            used += groups[g2].n;
                        }
                    }
                    for (size_t f = 0; f < phases.size(); f++) {
                        if (f + 1 == phases.size() && !imports.empty()) {  // imports run before the last phase's rounds
                            for (WJob &w : imports) w.phase = f == 0 ? kJobBefore : (uint8_t)(f - 1);
                            add_pass(g, imports);
                        }
                        for (uint32_t g2 : phases[f]) {
                            const Group &gr = groups[g2];
                            js.push_back(mkjob(ph.size(), gr.n, kJobLds, f, pslots + g2, i));
                            for (uint32_t q = 0; q < gr.n; q++) ph.push_back(slotted(pieces[gr.first + q], ph.size()));
                        }
                        close_phase(g, ph, lo);
                        if (f + 1 == phases.size() && js.size() == 1) break;  // the last phase's only group: added by the final job itself
                        add_pass(g, js);
                    }
                    std::vector<WJob> fin{mkjob(pslots, G, out_kind, phases.size() - 1, out_dst, i)};
                    if (js.size() == 1) {  // ... its pieces first (into its sum slot), then the groups' sums: one job, no barrier in between
                        fin[0].src2 = js[0].src; fin[0].n2 = js[0].n; fin[0].dst2 = (uint8_t)js[0].dst;
                        js.clear();
                    }
                    add_pass(g, fin);
                    finishers.push_back(std::move(g));
                }
            }
        }
        // whole rows and one-group units, packed: independent ones first (longest first), then by the age of what they wait for
        {
            std::vector<uint32_t> order(packs.size());
            for (uint32_t x = 0; x < order.size(); x++) order[x] = x;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                const Pack &a = packs[x], &b = packs[y];
                if ((a.dep != 0) != (b.dep != 0)) return a.dep == 0;
                if (a.dep != b.dep) return a.dep < b.dep;
                return a.n > b.n;
            });
            std::vector<char> taken(packs.size(), 0);
            size_t head = 0;
            // items per phase (a longer one-group unit has a phase to itself): one round where minibatches are small -- they are
            // latency, a second round of whole rows waits behind the first (cora: -15 %); all piece slots where throughput counts
            const uint32_t rounds = c->wide_rounds ? c->wide_rounds : (batch <= 512u ? 1u : 64u);
            const uint32_t cap = (uint32_t)std::min<uint64_t>(pslots, (uint64_t)rounds * ipb);
            while (head < order.size()) {
                Prog g;
                std::vector<Piece> ph;
                std::vector<WJob> js;
                for (uint32_t f = 0; f < std::max(1u, c->wide_phases); f++) {
                    size_t scanned = 0;
                    for (size_t x = head; x < order.size() && ph.size() < cap && scanned < 64; x++) {
                        if (taken[order[x]]) continue;
                        scanned++;
                        const Pack &pk = packs[order[x]];
                        if (ph.size() + pk.n > cap && !(ph.empty() && pk.n <= pslots)) continue;
                        taken[order[x]] = 1;
                        if (!(pieces[pk.first].it.flags & kItemDirect))
                            js.push_back(mkjob(ph.size(), pk.n, pk.kind, f, pk.dst, pk.row));
                        for (uint32_t q = 0; q < pk.n; q++) ph.push_back(slotted(pieces[pk.first + q], ph.size()));
                    }
                    while (head < order.size() && taken[order[head]]) head++;
                    if (ph.empty()) break;
                    close_phase(g, ph, lo);
                    add_pass(g, js);
                }
                if (!g.items.empty()) packed.push_back(std::move(g));
            }
        }
        // descriptors: helpers, finishers, packed
        auto emit = [&](std::vector<Prog> &v) {
            for (Prog &g : v) {
                WideDesc d{};
                d.lo = lo;
                d.index = b0 + k;
                d.kind = 0;
                d.a = (uint32_t)out.items.size();
                d.b = (uint32_t)(g.items.size() / ipb);
                d.c = (uint32_t)out.jobs.size();
                d.d = (uint32_t)g.jobs.size();
                out.items.insert(out.items.end(), g.items.begin(), g.items.end());
                out.jobs.insert(out.jobs.end(), g.jobs.begin(), g.jobs.end());
                out.wide.push_back(d);
                mb_items += (uint32_t)g.items.size();
                p.n_wgs++;
            }
        };
        p.n_helpers += (uint32_t)helpers.size();
        p.n_finishers += (uint32_t)finishers.size();
        p.n_packed += (uint32_t)packed.size();
        // (a unit's helpers come before its finisher -- it waits for their sums; where the whole-row workgroups go is free)
        if (c->wide_order == 2) emit(packed);
        emit(helpers);
        if (c->wide_order == 1) emit(packed);
        emit(finishers);
        if (c->wide_order == 0) emit(packed);
        // the combine trees above the units of rows with more than F*F pieces, level by level
        const uint32_t fin_first = (uint32_t)out.hubs.size();
        uint32_t fin_n = 0;
        for (int level = 0; !cur.empty(); level++) {
            nxt.clear();
            for (const Node &nd : cur) {
                const uint32_t G = (level == kMaxFinLevels - 1) ? nd.n : F;
                const uint32_t nout = (nd.n + G - 1) / G;
                if (nout == 1) {
                    out.hubs.push_back(FinItem{nd.in_slot, nd.n, kFinToStage, nd.row});
                    fin_n++;
                } else {
                    for (uint32_t o = 0; o < nout; o++) {
                        out.hubs.push_back(FinItem{nd.in_slot + o * G, std::min(G, nd.n - o * G), slots + o, nd.row});
                        fin_n++;
                    }
                    nxt.push_back(Node{nd.row, slots, nout});
                    slots += nout;
                }
            }
            cur.swap(nxt);
        }
        while (fin_n % 4u != 0) { out.hubs.push_back(FinItem{0, 0, kFinToStage, 0}); fin_n++; }
        for (uint32_t wn = 0; wn < fin_n / 4u; wn++) {
            WideDesc d{};
            d.lo = lo;
            d.index = b0 + k;
            d.kind = 1;
            d.a = fin_first;
            d.b = fin_n;
            d.c = wn;
            out.wide.push_back(d);
            p.n_wgs++;
            p.n_node_wgs++;
        }
        p.nnz += nnz;
        if (c->count_compulsory) p.compulsory += compulsory_bytes(c, seen, lo, hi, walk, nnz, mb_items);
    }
    p.n_slots = slots;
    return p;
}

// a built plan joins the handle's resident arrays
const WidePlan &wide_plan_append(f2v_ctx *c, uint32_t b0, uint32_t K, uint32_t batch, bool walk, WidePlan p, const WideParts &parts) {
    p.item_off = c->plan_items.h.size();
    p.fin_off = c->plan_hubs.h.size();
    p.wg_off = c->plan_wide.h.size();
    p.job_off = c->plan_jobs.h.size();
    c->plan_items.h.insert(c->plan_items.h.end(), parts.items.begin(), parts.items.end());
    c->plan_jobs.h.insert(c->plan_jobs.h.end(), parts.jobs.begin(), parts.jobs.end());
    c->plan_wide.h.insert(c->plan_wide.h.end(), parts.wide.begin(), parts.wide.end());
    c->plan_hubs.h.insert(c->plan_hubs.h.end(), parts.hubs.begin(), parts.hubs.end());
    // (the helpers' group sums are imported at 32-bit byte offsets: load16_agent)
    if (p.n_slots > kItemSlotMask || (uint64_t)p.n_slots * c->D * sizeof(float) > 0xFFFFFFFFull) c->plan_overflow = true;
    c->max_slots = std::max<size_t>(c->max_slots, p.n_slots);
    return c->wides.emplace(std::make_tuple(b0, K, batch, walk ? 1 : 0), p).first->second;
}

const WidePlan &wide_plan_for(f2v_ctx *c, uint32_t b0, uint32_t K, uint32_t batch, bool walk) {
    auto itp = c->wides.find(std::make_tuple(b0, K, batch, walk ? 1 : 0));
    if (itp != c->wides.end()) return itp->second;
    if (c->plan_items.h.size() > plan_cache_limit(c)) drop_plans(c);
    WideParts parts;
    const WidePlan p = build_wide_plan(c, b0, K, batch, walk, parts, c->seen_scratch);
    return wide_plan_append(c, b0, K, batch, walk, p, parts);
}

// Every wide-form plan of an epoch (launch l covers minibatches [l*K, l*K + K)): the missing ones are built side by side on the
// host's threads -- a plan reads the graph and the handle's parameters only -- and appended in launch order, so that the resident
// arrays are the ones a serial build leaves (F2V_IO_THREADS bounds the threads; a thread that counts compulsory bytes holds 4 N bytes
// of stamps).
void wide_plans_for_epoch(f2v_ctx *c, uint32_t nb, uint32_t K, uint32_t batch, bool walk, unsigned force_threads = 0) {
    std::vector<uint32_t> todo;
    for (uint32_t b0 = 0; b0 < nb; b0 += K)
        if (!c->wides.count(std::make_tuple(b0, std::min(K, nb - b0), batch, walk ? 1 : 0))) todo.push_back(b0);
    if (todo.empty()) return;
    if (c->plan_items.h.size() > plan_cache_limit(c)) {
        drop_plans(c);
        todo.clear();
        for (uint32_t b0 = 0; b0 < nb; b0 += K) todo.push_back(b0);
    }
    unsigned T = std::thread::hardware_concurrency();
    if (const char *e = getenv("F2V_IO_THREADS")) T = (unsigned)atoi(e);
    T = std::max(1u, std::min<unsigned>({T, 32u, (unsigned)todo.size()}));
    if (c->count_compulsory) T = std::min<unsigned>(T, std::max<unsigned>(1u, (unsigned)((1ull << 30) / std::max<uint64_t>(4ull * c->n, 1))));  // <= 1 GiB of stamps
    if (force_threads) T = std::max(2u, std::min<unsigned>(force_threads, (unsigned)todo.size()));  // (the self-test hook: the threaded path on any graph)
    if (T == 1 || (!force_threads && (uint64_t)c->nnz < (1ull << 22))) {  // small graphs: a thread costs more than the plan
        for (uint32_t b0 : todo) (void)wide_plan_for(c, b0, std::min(K, nb - b0), batch, walk);
        return;
    }
    const bool timing = getenv("F2V_PLAN_TIMING") != nullptr;  // (measurements: where the first call of a batch size spends its host time)
    const auto t_0 = std::chrono::steady_clock::now();
    std::vector<WideParts> parts(todo.size());
    std::vector<WidePlan> plans(todo.size());
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++)
        th.emplace_back([&] {
            SeenScratch seen;
            for (size_t k; (k = next.fetch_add(1)) < todo.size();)
                plans[k] = build_wide_plan(c, todo[k], std::min(K, nb - todo[k]), batch, walk, parts[k], seen);
        });
    for (auto &y : th) y.join();
    const auto t_1 = std::chrono::steady_clock::now();
    // the resident arrays get their final size once (no regrowth copies), the parts are moved in by the threads -- side by side: every
    // part has its place (prefix sums of the sizes), and a part is released as soon as it has been copied
    std::vector<size_t> at_items(todo.size() + 1, c->plan_items.h.size()), at_jobs(todo.size() + 1, c->plan_jobs.h.size()), at_wide(todo.size() + 1, c->plan_wide.h.size()),
        at_hubs(todo.size() + 1, c->plan_hubs.h.size());
    for (size_t k = 0; k < todo.size(); k++) {
        at_items[k + 1] = at_items[k] + parts[k].items.size();
        at_jobs[k + 1] = at_jobs[k] + parts[k].jobs.size();
        at_wide[k + 1] = at_wide[k] + parts[k].wide.size();
        at_hubs[k + 1] = at_hubs[k] + parts[k].hubs.size();
    }
    c->plan_items.h.resize(at_items.back());
    c->plan_jobs.h.resize(at_jobs.back());
    c->plan_wide.h.resize(at_wide.back());
    c->plan_hubs.h.resize(at_hubs.back());
    const auto t_2 = std::chrono::steady_clock::now();
    next = 0;
    th.clear();
    for (unsigned t = 0; t < T; t++)
        th.emplace_back([&] {
            for (size_t k; (k = next.fetch_add(1)) < todo.size();) {
                WideParts &q = parts[k];
                if (!q.items.empty()) memcpy(c->plan_items.h.data() + at_items[k], q.items.data(), q.items.size() * sizeof(Item));
                if (!q.jobs.empty()) memcpy(c->plan_jobs.h.data() + at_jobs[k], q.jobs.data(), q.jobs.size() * sizeof(WJob));
                if (!q.wide.empty()) memcpy(c->plan_wide.h.data() + at_wide[k], q.wide.data(), q.wide.size() * sizeof(WideDesc));
                if (!q.hubs.empty()) memcpy(c->plan_hubs.h.data() + at_hubs[k], q.hubs.data(), q.hubs.size() * sizeof(FinItem));
                q = WideParts{};
            }
        });
    for (auto &y : th) y.join();
    for (size_t k = 0; k < todo.size(); k++) {
        WidePlan &p = plans[k];
        p.item_off = at_items[k];
        p.job_off = at_jobs[k];
        p.wg_off = at_wide[k];
        p.fin_off = at_hubs[k];
        if (p.n_slots > kItemSlotMask || (uint64_t)p.n_slots * c->D * sizeof(float) > 0xFFFFFFFFull) c->plan_overflow = true;
        c->max_slots = std::max<size_t>(c->max_slots, p.n_slots);
        c->wides.emplace(std::make_tuple(todo[k], std::min(K, nb - todo[k]), batch, walk ? 1 : 0), p);
    }
    if (timing) {
        const auto t_3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "f2v plan timing: %zu plans on %u threads: built %.0f ms, resident arrays sized %.0f ms, parts moved in %.0f ms (%.1f MB of items)\n", todo.size(), T, ms(t_0, t_1), ms(t_1, t_2),
                ms(t_2, t_3), c->plan_items.h.size() * sizeof(Item) / 1e6);
    }
}

// Make every plan built so far resident in HBM (and the partial-sum buffer large enough).
int upload_plans(f2v_ctx *c) {
    if (c->plan_overflow) {
        c->plan_overflow = false;
        drop_plans(c);
        return fail(F2V_EINVAL, "a launch plan needs more than 2^28 partial-sum slots (or, in the wide form, 4 GiB of them): use a larger \"hub_chunk\" or fewer \"chain_rows\" / \"wide_rows\"");
    }
    const size_t need_slots = c->max_slots;
    const bool grow_slots = need_slots > c->d_ready.cap;  // (d_partials holds D floats for each of d_ready's slots)
    if (c->plan_items.h.size() == c->plan_items.resident && c->plan_hubs.h.size() == c->plan_hubs.resident && c->plan_wg.h.size() == c->plan_wg.resident &&
        c->plan_wide.h.size() == c->plan_wide.resident && c->plan_jobs.h.size() == c->plan_jobs.resident && !grow_slots)
        return F2V_OK;  // O(1) steady state
    HIPC(hipStreamSynchronize(c->stream));  // launches in flight read these buffers
    const auto t_up0 = std::chrono::steady_clock::now();
    F2VC(c->plan_wide.upload(1024));
    F2VC(c->plan_jobs.upload(1024));
    F2VC(c->plan_wg.upload(1024));
    F2VC(c->plan_items.upload(1024));
    F2VC(c->plan_hubs.upload(256));
    if (grow_slots) {
        F2VC(c->d_partials.reserve(need_slots * (size_t)c->D, "partial sums"));
        F2VC(c->d_ready.reserve(need_slots, "partial sums"));
        // hipMemset on device memory may return before the fill has run (it is ordered on the NULL stream, which this
        // engine's non-blocking stream does not wait for): a late fill would wipe the first launch's flags
        HIPC(hipMemsetAsync(c->d_ready, 0, need_slots * sizeof(uint32_t), c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    if (getenv("F2V_PLAN_TIMING"))
        fprintf(stderr, "f2v plan timing: upload %.0f ms (resident: %zu items, %zu tree nodes, %zu chain workgroups, %zu wide workgroups, %zu jobs, %zu partial-sum slots)\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up0).count(), c->plan_items.d.cap, c->plan_hubs.d.cap,
                c->plan_wg.d.cap, c->plan_wide.d.cap, c->plan_jobs.d.cap, c->d_ready.cap);
    return F2V_OK;
}

template <int VEC, bool EXACT>
void launch_commit_t(f2v_ctx *c, uint32_t lo, uint32_t rows) {
    const int wpb = 4;
    const uint32_t blocks = std::min<uint32_t>((rows + wpb - 1) / wpb, 4096u);
    hipLaunchKernelGGL((commit_kernel<VEC, EXACT>), dim3(blocks), dim3(64 * wpb), 0, c->stream, c->d_X[c->cur], c->d_X[c->cur ^ 1], lo, rows, c->D);
}

template <typename F>
int dispatch_layout(f2v_ctx *c, F &&f) {
    // (VEC, EXACT) instantiations: exact vector loads when D == 64*VEC, guarded scalar loads otherwise
    if (c->exact) {
        switch (c->vec) {
            case 1: f(std::integral_constant<int, 1>{}, std::true_type{}); return F2V_OK;
            case 2: f(std::integral_constant<int, 2>{}, std::true_type{}); return F2V_OK;
            case 4: f(std::integral_constant<int, 4>{}, std::true_type{}); return F2V_OK;
            case 8: f(std::integral_constant<int, 8>{}, std::true_type{}); return F2V_OK;
        }
    } else {
        switch (c->vec) {
            case 1: f(std::integral_constant<int, 1>{}, std::false_type{}); return F2V_OK;
            case 2: f(std::integral_constant<int, 2>{}, std::false_type{}); return F2V_OK;
            case 4: f(std::integral_constant<int, 4>{}, std::false_type{}); return F2V_OK;
            case 8: f(std::integral_constant<int, 8>{}, std::false_type{}); return F2V_OK;
        }
    }
    return fail(F2V_EINVAL, "unsupported dimension %u", c->D);
}

// ... and f(OPT, VEC, EXACT) for the kernels of the generic layout that differ by the option's math (5, or 6: math 7 runs 6)
template <typename F>
int dispatch_math_layout(f2v_ctx *c, int math, F &&f) {
    return dispatch_layout(c, [&](auto V, auto E) {
        if (math == 5) f(Int<5>{}, V, E);
        else f(Int<6>{}, V, E);
    });
}

// Make d_X[cur] the whole, up-to-date matrix: a completed epoch (all N rows updated) just swaps the two
// matrices; a partial range is folded back with a copy.
int flush_pending(f2v_ctx *c) {
    c->pending = false;
    if (c->upd_hi == c->upd_lo) return F2V_OK;
    if (c->upd_lo == 0 && c->upd_hi == c->n) {
        c->cur ^= 1;
    } else {
        const uint32_t lo = c->upd_lo, rows = c->upd_hi - c->upd_lo;
        int rc = dispatch_layout(c, [&](auto V, auto E) { launch_commit_t<decltype(V)::value, decltype(E)::value>(c, lo, rows); });
        if (rc != F2V_OK) return rc;
        HIPC(hipGetLastError());
    }
    c->upd_lo = c->upd_hi = 0;
    return F2V_OK;
}

// What every call that reads the settled matrix begins with: the embeddings exist, the handle's device is current, the minibatches
// stepped so far are folded in.  (Each call's own range checks stand before or after it, in the order its errors are documented.)
int settled_enter(f2v_ctx *c, const char *who) {
    if (!c->have_x)
        return fail(F2V_ESTATE, c->x_invalid ? "%s: the embeddings are invalid since a launch gave up a bounded wait: set or initialise them again"
                                             : "%s: embeddings were never initialised", who);
    HIPC(hipSetDevice(c->device));
    return flush_pending(c);
}

// More than 64 KiB of dynamic LDS has to be allowed per kernel.  The limit belongs to the kernel on its device, not to a handle, and so
// does the record of what it has been raised to: one entry per kernel instantiation, raised when a launch needs more than any launch
// before it and never lowered, whichever handle asks.
int allow_lds(f2v_ctx *c, const void *kernel, size_t bytes) {
    static std::mutex mutex;
    static std::map<std::pair<int, const void *>, size_t> granted;
    if (bytes <= 64 * 1024) return F2V_OK;
    std::lock_guard<std::mutex> lock(mutex);
    size_t &limit = granted[{c->device, kernel}];
    if (bytes <= limit) return F2V_OK;
    HIPC(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    limit = bytes;
    return F2V_OK;
}

// ---- the training objective (f2v_objective, "loss_every") ---------------------------------------------------------------------
int math_of_option(int option);

// The whole matrix as it stands without folding anything back: d_X[cur] when nothing is pending, the second matrix after a completed
// epoch (every row updated); nullptr otherwise (flush first).
const float *settled_matrix(const f2v_ctx *c) {
    if (c->upd_hi == c->upd_lo) return c->d_X[c->cur];
    if (c->upd_lo == 0 && c->upd_hi == c->n) return c->d_X[c->cur ^ 1];
    return nullptr;
}

uint64_t mix64_host(uint64_t z) {  // f2v_kernels.hip.h: mix64
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The objective kernel's items (every row cut into pieces of at most kObjChunk neighbours; the last piece of a row, also of a row
// without neighbours, takes its negative samples), sorted by neighbour count, longest first, ties in row order -- a function of
// rowptr alone -- and the buffers of its results.  Once per handle, outside every timed loop.
int objective_prepare(f2v_ctx *c) {
    if (c->d_obj_items) return F2V_OK;
    std::vector<uint32_t> count(kObjChunk + 1, 0);
    uint64_t total = 0;
    for (uint32_t r = 0; r < c->n; r++) {
        const uint32_t deg = c->rowptr[r + 1] - c->rowptr[r];
        const uint32_t pieces = deg ? (deg + kObjChunk - 1) / kObjChunk : 1u;
        total += pieces;
        count[kObjChunk] += pieces - 1;
        count[deg ? deg - (pieces - 1) * kObjChunk : 0]++;
    }
    if (total > 0xFFFFFFFFull - kObjItemsPerWg) return fail(F2V_EINVAL, "f2v_objective: %llu work items are too many", (unsigned long long)total);
    std::vector<uint32_t> start(kObjChunk + 1, 0);  // counting sort, longest first
    for (int k = (int)kObjChunk - 1; k >= 0; k--) start[k] = start[k + 1] + count[k + 1];
    std::vector<Item> items(total);
    for (uint32_t r = 0; r < c->n; r++) {
        const uint32_t rp = c->rowptr[r], deg = c->rowptr[r + 1] - rp;
        const uint32_t pieces = deg ? (deg + kObjChunk - 1) / kObjChunk : 1u;
        for (uint32_t p = 0; p < pieces; p++) {
            const uint32_t cnt = std::min(kObjChunk, deg - p * kObjChunk);
            items[start[cnt]++] = Item{r, rp + p * kObjChunk, cnt, p + 1 == pieces ? kItemLast : 0u};
        }
    }
    const uint32_t wgs = (uint32_t)((total + kObjItemsPerWg - 1) / kObjItemsPerWg);
    F2VC(c->d_obj_part.reserve(wgs, "objective"));
    F2VC(c->d_obj_out.reserve(kLossLogMax + 1, "objective"));
    F2VC(c->d_obj_items.reserve(total, "objective"));  // (the last one: its presence says that all three exist)
    if (total) HIPC(hipMemcpy(c->d_obj_items, items.data(), total * sizeof(Item), hipMemcpyHostToDevice));
    c->obj_items = (uint32_t)total;
    return F2V_OK;
}

template <int SIG, int VEC, bool EXACT>
void launch_objective_t(f2v_ctx *c, const ObjArgs &a, uint32_t wgs) {
    hipLaunchKernelGGL((objective_kernel<SIG, VEC, EXACT>), dim3(wgs), dim3(64 * 4), 0, c->stream, a);
}

// Enqueue one evaluation of matrix X (two launches, no synchronisation, no allocation): *out receives the sums.
int launch_objective(f2v_ctx *c, const float *X, int option, uint32_t ns, ObjPartial *out) {
    ObjArgs a{};
    a.X = X;
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.items = c->d_obj_items;
    a.part = c->d_obj_part;
    a.seed_mix = mix64_host(c->loss_seed);
    a.n_items = c->obj_items;
    a.n = c->n;
    a.D = c->D;
    a.ns = ns;
    a.unit_degi = option == 10 ? 1u : 0u;
    const bool sig = math_of_option(option) != 5;
    const uint32_t wgs = (c->obj_items + kObjItemsPerWg - 1) / kObjItemsPerWg;
    if (wgs) {
        int rc = dispatch_layout(c, [&](auto V, auto E) {
            if (sig) launch_objective_t<1, decltype(V)::value, decltype(E)::value>(c, a, wgs);
            else launch_objective_t<0, decltype(V)::value, decltype(E)::value>(c, a, wgs);
        });
        if (rc != F2V_OK) return rc;
        HIPC(hipGetLastError());
    }
    hipLaunchKernelGGL(objective_reduce_kernel, dim3(1), dim3(1024), 0, c->stream, (const ObjPartial *)c->d_obj_part, wgs, out);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// A combine-tree node's wait timed out (the words of d_kerr are in `e`): nodes that give up store nothing, so the rows
// of the affected hub vertices were not updated from that launch on -- the embeddings are invalid and must be set again.
// The handle stays usable: the error words are cleared and it runs one launch per tree level from now on (no in-grid waits).
int kernel_gave_up(f2v_ctx *c, const char *where, const uint32_t *e) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemsetAsync(c->d_kerr, 0, 64, c->stream);
    (void)hipStreamSynchronize(c->stream);
    c->merge_fin = false;  // (chained minibatches need it: off with it)
    c->pending = false;
    c->upd_lo = c->upd_hi = 0;
    c->have_x = false;
    c->x_invalid = true;
    if (e[0] == 4u)  // a finisher's import: err[2] waiting workgroup, [3] partial-sum slot, [4] flag seen, [5] launch, [6] grid, [7] the minibatch's first row
        return fail(F2V_ESTATE, "%s: a chained launch was lost: %u waits for a helper's group sum gave up (first: workgroup %u of %u, minibatch starting at row %u, "
                    "partial-sum slot %u: flag %u, launch %u); the embeddings are invalid from that launch on (set or initialise them again); this handle now runs one "
                    "launch per minibatch and per combine-tree level (\"merge_finalize\" = 0)",
                    where, e[1], e[2], e[6], e[7], e[3], e[4], e[5]);
    if (e[0] == 3u)  // wait_row_slow: err[2] waiting workgroup, [3] row, [4] flag seen, [5] launch, [6] grid, [7] the minibatch's first row
        return fail(F2V_ESTATE, "%s: a chained launch was lost: %u row waits gave up (first: workgroup %u of %u, minibatch starting at row %u, waiting for row %u: "
                    "flag %u, launch %u); the embeddings are invalid from that launch on (set or initialise them again); this handle now runs one launch "
                    "per minibatch and per combine-tree level (\"merge_finalize\" = 0)",
                    where, e[1], e[2], e[6], e[7], e[3], e[4], e[5]);
    return fail(F2V_ESTATE, "%s: %u combine-tree waits gave up (first: node %u of %u [first dependent %u] on slot %u, flag %u, launch %u); "
                "the embeddings are invalid from that minibatch on (set or initialise them again); this handle now runs with \"merge_finalize\" = 0",
                where, e[1], e[2], e[6], e[7], e[3], e[4], e[5]);
}

// after a stream synchronisation: did a kernel give up a bounded wait?
int check_kernel_err(f2v_ctx *c, const char *where) {
    uint32_t e[8] = {};
    HIPC(hipMemcpy(e, c->d_kerr, sizeof e, hipMemcpyDeviceToHost));
    if (e[0]) return kernel_gave_up(c, where, e);
    return F2V_OK;
}

int math_of_option(int option) {
    switch (option) {
        case 5: case 8: case 11: return 5;
        case 6: case 9: return 6;
        case 7: case 10: return 7;
        default: return 0;
    }
}

// Launch one minibatch step (+ hub finalisation) on the handle's stream.  d_ids: device sample ids.
void fill_targets(const f2v_ctx *c, PushTargets &t, int which, uint32_t batch_lo, const uint32_t *d_masks);

// a bound given in milliseconds in ticks of the 100 MHz wall clock (wall_clock64)
unsigned long long ms_to_ticks(int64_t ms) { return (unsigned long long)ms * 100000ull; }

// bound of a combine-tree node's wait ("tree_timeout_ms", default 5 s; the environment variable F2V_TREE_TIMEOUT_MS sets the
// default of new handles)
unsigned long long tree_timeout_ticks(const f2v_ctx *c) { return ms_to_ticks(c->tree_timeout_ms); }

// the sequence number of a launch with in-grid waits (never 0: that is what fresh flags hold)
uint32_t next_launch_seq(f2v_ctx *c) {
    if (++c->launch_seq == 0) ++c->launch_seq;
    return c->launch_seq;
}

// a launch whose first row is `lo` does not continue the updated range (a new epoch, or batches out of order): swap / fold first
int flush_unless_continued(f2v_ctx *c, uint32_t lo) { return (c->upd_hi != c->upd_lo && lo != c->upd_hi) ? flush_pending(c) : F2V_OK; }

// the first row a chained launch starting at row `lo` reads from the second matrix
uint32_t chain_upd_lo(const f2v_ctx *c, uint32_t lo) { return c->upd_hi == c->upd_lo ? lo : c->upd_lo; }

// what every form of the step kernel is told: the matrices, the graph, the launch's items, the step's scalars
void fill_step_args(const f2v_ctx *c, StepArgs &a, int math, size_t item_off, uint32_t upd_lo, uint32_t ns, float lr, int bs_mode) {
    a.X = c->d_X[c->cur];
    a.Xn = c->d_X[c->cur ^ 1];
    a.rowptr = c->d_rowptr;
    a.nbr_ids = math == 7 ? c->d_walks : c->d_colids;
    a.partials = c->d_partials;
    a.items = c->plan_items.d + item_off;
    a.sm_table = c->d_table;
    a.D = c->D;
    a.upd_lo = upd_lo;
    a.ns = ns;
    a.bs_mode = bs_mode ? 1u : 0u;
    a.unit_degi = c->unit_degi ? 1u : 0u;
    a.lr = lr;
}

// Arm the in-grid waits of a launch: the flags, where a wait that gives up reports, its bound and a fresh sequence number.
// A chained launch lasts a millisecond or two: its waits are bounded by "chain_timeout_ms" as well.
void arm_waits(f2v_ctx *c, StepArgs &a, bool chained) {
    a.ready = c->d_ready;
    a.err = c->d_kerr;
    a.timeout_ticks = chained ? ms_to_ticks(std::min(c->tree_timeout_ms, c->chain_timeout_ms)) : tree_timeout_ticks(c);
    a.seq = next_launch_seq(c);
}

// The self-test build's hook fields of a launch (include/f2v_test.h).  Row waits switched off: the wide form reads the mode's bits,
// the chain form is told that no row was "written by an earlier minibatch" (chain_lo = 0xFFFFFFFF).
#ifdef F2V_TEST_HOOKS
void fill_hooks(const f2v_ctx *c, StepArgs &a, bool chained, bool wide) {
    const f2v_ctx::Hooks &h = c->hooks;
    a.test_withhold_slot = h.withhold_slot;
    a.test_withhold_row = chained ? h.withhold_row : kNoSlot;
    a.stamps = chained ? h.d_stamps : nullptr;
    a.xcd_times = chained ? nullptr : h.d_xcd;
    a.test_stub = chained ? 0u : h.stub;
    a.test_nowait = wide ? h.chain_mode : 0u;
    if (chained && !wide && (h.chain_mode & 1u)) a.chain_lo = 0xFFFFFFFFu;
}
bool hooks_forbid_ring(const f2v_ctx *c) { return c->hooks.d_stamps || c->hooks.chain_mode; }  // (they look at one epoch per launch)
#else
void fill_hooks(const f2v_ctx *, StepArgs &, bool, bool) {}
bool hooks_forbid_ring(const f2v_ctx *) { return false; }
#endif

// Record a launch over rows [lo, hi) that computed `rows` rows against `samples` negative samples, `epochs` times over: the
// statistics and -- unless nothing is left pending (the ring of the wide form) -- the updated range, with [p_lo, hi) the last minibatch
template <class P>
void record_launch(f2v_ctx *c, const P &plan, uint32_t lo, uint32_t hi, uint32_t p_lo, uint64_t rows, uint64_t samples, uint64_t epochs = 1,
                   bool pending = true) {
    if (pending) {
        if (c->upd_hi == c->upd_lo) c->upd_lo = lo;
        c->upd_hi = hi;
        c->pending = true;
        c->p_lo = p_lo;
        c->p_hi = hi;
    }
    // statistics: algorithmic bytes of SURVEY 8d -- nnz*(4D+4) + rows*(8D+4) + ns*(4D+4) per minibatch
    c->stats.hub_rows += (uint64_t)plan.n_hubs * epochs;
    c->stats.hub_chunks += (uint64_t)plan.n_chunks * epochs;
    c->stats.step_launches += 1;
    c->stats.rows += rows * epochs;
    c->stats.nnz += plan.nnz * epochs;
    c->stats.algorithmic_bytes += (plan.nnz * (4ull * c->D + 4) + rows * (8ull * c->D + 4) + samples * (4ull * c->D + 4)) * epochs;
    c->stats.compulsory_bytes += plan.compulsory * epochs;
}

// `epochs` epochs of seven counters as `per` of them counted (f2v_train's hipGraph form counts two while it captures)
void scale_stats(f2v_stats &s, uint64_t epochs, uint64_t per) {
    for (uint64_t *v : {&s.step_launches, &s.rows, &s.nnz, &s.algorithmic_bytes, &s.hub_rows, &s.hub_chunks, &s.compulsory_bytes}) *v = *v / per * epochs;
}

// combine-tree launch of `n` nodes at `items`, reading and writing what the step launch `a` did
FinalizeArgs finalize_args(const f2v_ctx *c, const StepArgs &a, const FinItem *items, uint32_t n) {
    FinalizeArgs f{};
    f.X = a.X;
    f.partials = c->d_partials;
    f.Xn = a.Xn;
    f.items = items;
    f.n_items = n;
    f.D = c->D;
    f.push = a.push;
    return f;
}

// push_masks / push: a sharded run's step -- the kernels also store every finished row into the second matrix of
// the peers that read it (push_masks == nullptr: of every peer).
int launch_step(f2v_ctx *c, int math, uint32_t batch_lo, uint32_t batch_hi, uint32_t row_lo, uint32_t row_hi,
                const uint32_t *d_ids, uint32_t ns, float lr, int bs_mode, bool push = false, const uint32_t *push_masks = nullptr) {
    int rc;
    if ((rc = flush_unless_continued(c, batch_lo)) != F2V_OK) return rc;
    const Plan plan = plan_for(c, row_lo, row_hi, math == 7);  // by value: upload_plans may not move it, but keep it simple
    if ((rc = upload_plans(c)) != F2V_OK) return rc;
    StepArgs a{};
    fill_step_args(c, a, math, plan.item_off, c->upd_lo, ns, lr, bs_mode);
    a.sample_ids = d_ids;
    a.batch_lo = batch_lo;
    a.n_items = plan.n_items;
    a.upd_rows = c->upd_hi - c->upd_lo;
    fill_hooks(c, a, false, false);
    push = push && c->push.attached && c->push.world > 1;
    if (push) fill_targets(c, a.push, c->cur ^ 1, batch_lo, push_masks);

    const uint32_t wpb = (uint32_t)c->waves_per_block;
    // sub-wave layout when D is a multiple of 4 up to 256: 16, 8 or 4 work items per wavefront
    const uint32_t width = subwave_width(c);
    const bool quarter = width != 0;
    const uint32_t per_wave = items_per_wave(width);
    const uint32_t waves = (plan.n_items + per_wave - 1) / per_wave;
    uint32_t blocks = (waves + wpb - 1) / wpb;  // 0 when this rank has no row of the batch
    a.step_blocks = blocks;
    uint32_t tree_nodes = 0;
    for (int lev = 0; lev < plan.n_levels; lev++) tree_nodes += plan.fin_cnt[lev];  // the levels are stored back to back
    // sub-wave kernel: the combine trees ride in the same grid (one launch per minibatch)
    const bool fused_tree = quarter && c->merge_fin && !c->capturing && plan.n_levels >= 1 && blocks > 0;
    if (fused_tree) {
        a.fin_items = c->plan_hubs.d + plan.fin_off[0];
        a.fin_n = tree_nodes;
        arm_waits(c, a, false);
        blocks += (a.fin_n + wpb - 1) / wpb;
    }
    if (blocks == 0) {
        // nothing to compute here; the range bookkeeping below still advances
    } else if (quarter) {
        // rows in flight per item: 4 at D = 128 (90 VGPRs, 5 waves/SIMD; 8 is selectable and measured 3-9 % slower
        // on RMAT-20: 116 VGPRs, 4 waves/SIMD) and at D = 256; 8 where a row is a single dwordx4 per lane (D <= 64)
        rc = dispatch_subwave<16, true>(c, math, width, [&](auto O, auto L, auto N, auto U, auto FL) {
            constexpr int OPT = decltype(O)::value, LPI = decltype(L)::value, NB = decltype(N)::value, UR = decltype(U)::value;
            constexpr bool FULL = decltype(FL)::value;
            if (push) hipLaunchKernelGGL((qstep_kernel<OPT, LPI, NB, UR, true, FULL>), dim3(blocks), dim3(64 * wpb), 0, c->stream, a);
            else hipLaunchKernelGGL((qstep_kernel<OPT, LPI, NB, UR, false, FULL>), dim3(blocks), dim3(64 * wpb), 0, c->stream, a);
        });
        if (rc != F2V_OK) return rc;
    } else {
        rc = dispatch_math_layout(c, math, [&](auto O, auto V, auto E) {
            hipLaunchKernelGGL((step_kernel<decltype(O)::value, decltype(V)::value, decltype(E)::value>), dim3(blocks), dim3(64 * wpb), 0, c->stream, a);
        });
        if (rc != F2V_OK) return rc;
    }
    HIPC(hipGetLastError());
    const bool tree = !fused_tree && c->merge_fin && !c->capturing && plan.n_levels >= 2;
    if (tree) {
        FinalizeTreeArgs t{};
        t.f = finalize_args(c, a, c->plan_hubs.d + plan.fin_off[0], tree_nodes);
        t.ready = c->d_ready;
        t.err = c->d_kerr;
        t.timeout_ticks = tree_timeout_ticks(c);
        t.seq = next_launch_seq(c);
        t.first_dep = plan.fin_cnt[0];
        const uint32_t fb = (t.f.n_items + wpb - 1) / wpb;  // the node layout counts on `wpb` nodes per workgroup
        rc = dispatch_math_layout(c, math, [&](auto O, auto V, auto E) {
            hipLaunchKernelGGL((hub_finalize_tree_kernel<decltype(O)::value, decltype(V)::value, decltype(E)::value>), dim3(fb), dim3(64 * wpb), 0, c->stream, t);
        });
        if (rc != F2V_OK) return rc;
        HIPC(hipGetLastError());
    }
    for (int lev = 0; lev < plan.n_levels && !tree && !fused_tree; lev++) {
        const FinalizeArgs f = finalize_args(c, a, c->plan_hubs.d + plan.fin_off[lev], plan.fin_cnt[lev]);
        const uint32_t fb = (f.n_items + 3) / 4;
        rc = dispatch_math_layout(c, math, [&](auto O, auto V, auto E) {
            hipLaunchKernelGGL((hub_finalize_kernel<decltype(O)::value, decltype(V)::value, decltype(E)::value>), dim3(fb), dim3(256), 0, c->stream, f);
        });
        if (rc != F2V_OK) return rc;
        HIPC(hipGetLastError());
    }
    record_launch(c, plan, batch_lo, batch_hi, batch_lo, row_hi - row_lo, ns);
    return F2V_OK;
}

// the fields the two chained forms share: the tree nodes, the armed waits, the rows handed on inside the launch
template <class P>
void fill_chain_args(f2v_ctx *c, StepArgs &a, int math, const P &plan, uint32_t ns, float lr, int bs_mode) {
    fill_step_args(c, a, math, plan.item_off, chain_upd_lo(c, plan.lo), ns, lr, bs_mode);
    a.fin_items = c->plan_hubs.d + plan.fin_off;
    arm_waits(c, a, true);
    a.rowflag = c->d_rowflag;
    a.chain_lo = plan.lo;
    fill_hooks(c, a, true, std::is_same<P, WidePlan>::value);
}

// One chained launch: minibatches [plan.first_batch, +plan.n_batches) of an epoch whose sample ids (ids_stride per minibatch)
// lie at d_ids_epoch.
int launch_chain(f2v_ctx *c, int math, const ChainPlan &plan, const uint32_t *d_ids_epoch, uint32_t ids_stride, uint32_t ns, float lr, int bs_mode) {
    int rc;
    if ((rc = flush_unless_continued(c, plan.lo)) != F2V_OK) return rc;
    ChainArgs ca{};
    fill_chain_args(c, ca.base, math, plan, ns, lr, bs_mode);
    ca.wg = c->plan_wg.d + plan.wg_off;
    ca.ids = d_ids_epoch;
    ca.ids_stride = ids_stride;
    const uint32_t wpb = (uint32_t)c->waves_per_block;
    // (no 16-wide instance: rows narrower than a 128-byte line chain in the wide form only, chain_usable)
    rc = dispatch_subwave<32, true>(c, math, subwave_width(c), [&](auto O, auto L, auto N, auto U, auto FL) {
        hipLaunchKernelGGL((qstep_chain_kernel<decltype(O)::value, decltype(L)::value, decltype(N)::value, decltype(U)::value, decltype(FL)::value>),
                           dim3(plan.n_wgs), dim3(64 * wpb), 0, c->stream, ca);
    });
    if (rc != F2V_OK) return rc;
    HIPC(hipGetLastError());
    c->last_train_form = 1;
    record_launch(c, plan, plan.lo, plan.hi, plan.last_lo, plan.hi - plan.lo, (uint64_t)plan.n_batches * ns);
    return F2V_OK;
}

void free_ring(f2v_ctx *c) {
    c->d_ring.release();
    c->d_ring_partials.release();
    c->d_ring_flags.release();
    c->d_ring_ready.release();
}

// One launch of the wide form (qwide_chain_kernel): minibatches [plan.first_batch, +plan.n_batches)
// `epochs` > 1 (the plan covers the whole graph): that many epochs chained in the one launch -- the current matrix is copied into a ring
// of epochs + 1 matrices, epoch e reads matrix e and writes matrix e + 1 behind its own row flags, and the last one is copied back
// (two 1-MB copies per launch on a graph like cora, where the launch boundary they replace is a third of an epoch).
int launch_wide(f2v_ctx *c, int math, const WidePlan &plan, const uint32_t *d_ids_epoch, uint32_t ids_stride, uint32_t ns, float lr, int bs_mode,
                uint32_t *epochs_io = nullptr, uint64_t ids_epoch_stride = 0) {
    int rc;
    uint32_t epochs = epochs_io ? *epochs_io : 1u;
    if (epochs > 1 && (c->ring_epochs < epochs || c->ring_slots < std::max<size_t>(plan.n_slots, 1))) {
        // the ring of matrices (and the per-epoch flags and partial sums): where the device has no room for it, one epoch per launch
        HIPC(hipStreamSynchronize(c->stream));
        free_ring(c);
        const uint32_t cap = std::max(epochs, c->ring_epochs);
        const size_t slots = std::max<size_t>(std::max<size_t>(plan.n_slots, c->ring_slots), 1), mat = (size_t)c->n * c->D;
        c->ring_epochs = 0;
        c->ring_slots = 0;
        bool refuse = false;
#ifdef F2V_TEST_HOOKS
        refuse = getenv("F2V_TEST_RING_REFUSE") != nullptr;  // fault injection: as if the device had no room for the ring
#endif
        if (refuse || !c->d_ring.try_reserve((size_t)(cap + 1) * mat) || !c->d_ring_partials.try_reserve((size_t)cap * slots * c->D) ||
            !c->d_ring_flags.try_reserve((size_t)cap * c->n) || !c->d_ring_ready.try_reserve((size_t)cap * slots)) {
            free_ring(c);
            c->ring_refused = true;  // (f2v_train stops asking)
            epochs = 1;
        } else {
            HIPC(hipMemsetAsync(c->d_ring_flags, 0, (size_t)cap * c->n * sizeof(uint32_t), c->stream));  // 0 is no launch's sequence number
            HIPC(hipMemsetAsync(c->d_ring_ready, 0, (size_t)cap * slots * sizeof(uint32_t), c->stream));
            c->ring_epochs = cap;
            c->ring_slots = slots;
        }
    }
    if (epochs_io) *epochs_io = epochs;
    const bool ring = epochs > 1;
    if ((rc = ring ? flush_pending(c) : flush_unless_continued(c, plan.lo)) != F2V_OK) return rc;
    const size_t matrix = (size_t)c->n * c->D;
    if (ring) {
        if (plan.lo != 0 || plan.hi != c->n || plan.n_node_wgs != 0) return fail(F2V_ESTATE, "launch_wide: epochs can only be chained where one launch covers the graph");
        HIPC(hipMemcpyAsync(c->d_ring, c->d_X[c->cur], matrix * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    WideArgs wa{};
    StepArgs &a = wa.base;
    fill_chain_args(c, a, math, plan, ns, lr, bs_mode);
    if (ring) {  // the ring's matrices, and every epoch its own partial sums and flags
        a.X = c->d_ring;
        a.Xn = c->d_ring + matrix;
        a.partials = c->d_ring_partials;
        a.ready = c->d_ring_ready;
        a.rowflag = c->d_ring_flags;
        wa.wgs_per_epoch = plan.n_wgs;
        wa.n_rows = c->n;
        wa.slots_per_epoch = (uint32_t)c->ring_slots;
        wa.ring_stride = matrix;
        wa.ids_epoch_stride = ids_epoch_stride;
    }
    wa.wg = c->plan_wide.d + plan.wg_off;
    wa.jobs = c->plan_jobs.d + plan.job_off;
    wa.ids = d_ids_epoch;
    wa.ids_stride = ids_stride;
    // "wide_samples_early" (-1 = automatic): on for graphs of up to 2 M nonzeros, whose launches are one dependency chain
    const bool early = ring || (c->wide_samples_early >= 0 ? c->wide_samples_early != 0 : c->nnz <= (2ull << 20));
    c->last_wide_early = early;
    c->last_wide_width = plan.width;
    c->last_train_form = 2;
    c->last_wide_epochs = std::max(c->last_wide_epochs, epochs);  // (the most epochs one launch of this f2v_train has carried)
    const uint32_t grid = plan.n_wgs * epochs;
    // MODE 2: epochs chained through the ring; 1: the EARLY form; 0: the plain one.  Always the table's rows in flight.
    rc = dispatch_subwave<16, false>(c, math, plan.width, [&](auto O, auto L, auto N, auto U, auto FL) {
        constexpr int OPT = decltype(O)::value, LPI = decltype(L)::value, NB = decltype(N)::value, UR = decltype(U)::value;
        constexpr bool FULL = decltype(FL)::value;
        if (ring) hipLaunchKernelGGL((qwide_chain_kernel<OPT, LPI, NB, UR, FULL, 2>), dim3(grid), dim3(256), 0, c->stream, wa);
        else if (early) hipLaunchKernelGGL((qwide_chain_kernel<OPT, LPI, NB, UR, FULL, 1>), dim3(grid), dim3(256), 0, c->stream, wa);
        else hipLaunchKernelGGL((qwide_chain_kernel<OPT, LPI, NB, UR, FULL, 0>), dim3(grid), dim3(256), 0, c->stream, wa);
    });
    if (rc != F2V_OK) return rc;
    HIPC(hipGetLastError());
    if (ring)  // the last epoch's matrix becomes the current one: nothing is pending
        HIPC(hipMemcpyAsync(c->d_X[c->cur], c->d_ring + (size_t)epochs * matrix, matrix * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    record_launch(c, plan, plan.lo, plan.hi, plan.last_lo, plan.hi - plan.lo, (uint64_t)plan.n_batches * ns, epochs, !ring);
    return F2V_OK;
}

void generate_walks_host(f2v_ctx *c, std::vector<uint32_t> &walks) {
    // sample/algorithms.cpp:1097-1118, from the handle's rand() stream (f2v_host.cpp: walks_host)
    walks.resize((size_t)c->n * kWalkLength);
    walks_host(c->rng, c->rowptr.data(), c->colids.data(), c->n, c->nnz, walks.data());
}

// ---- push exchange helpers (include/f2v.h) ---------------------------------------------------------------
// slice of rank r of minibatch [lo,hi): contiguous; work-balanced over the CSR (f2v_shard_bounds), equal row counts
// for the walk-based option 7 (every row has five pairs)
void shard_of(const f2v_ctx *c, bool walk, uint32_t lo, uint32_t hi, uint32_t rank, uint32_t world, uint32_t *my_lo, uint32_t *my_hi) {
    if (walk) {
        const uint32_t per = (hi - lo + world - 1) / world;
        *my_lo = (uint32_t)std::min<uint64_t>((uint64_t)lo + (uint64_t)rank * per, hi);
        *my_hi = (uint32_t)std::min<uint64_t>((uint64_t)*my_lo + per, hi);
        return;
    }
    uint32_t bounds[kMaxRanks + 1];
    (void)f2v_shard_bounds(c->rowptr.data(), lo, hi, world, bounds);
    *my_lo = bounds[rank];
    *my_hi = bounds[rank + 1];
}

// where the peers receive rows of the minibatch that starts at `batch_lo`: their copy of matrix `which`, or the half of
// their landing buffer this exchange uses
void fill_targets(const f2v_ctx *c, PushTargets &t, int which, uint32_t batch_lo, const uint32_t *d_masks) {
    const auto &P = c->push;
    for (uint32_t r = 0; r < P.world; r++)
        t.peer[r] = P.landing ? P.peer_landing[r] + (size_t)(P.round & 1u) * P.landing_cap * c->D : P.peer_X[which][r];
    t.masks = d_masks;
    t.self = P.rank;
    t.world = P.world;
    t.row_base = P.landing ? batch_lo : 0u;
}

// copy my rows [row_lo,row_hi) of local matrix `which` to the peers that read them
int launch_push(f2v_ctx *c, int which, const uint32_t *d_masks, uint32_t batch_lo, uint32_t row_lo, uint32_t row_hi) {
    if (c->push.world < 2 || row_hi <= row_lo) return F2V_OK;
    PushArgs a{};
    a.src = c->d_X[which];
    fill_targets(c, a.to, which, batch_lo, d_masks);
    a.row_lo = row_lo;
    a.rows = row_hi - row_lo;
    a.D = c->D;
    const uint32_t wpb = 4;
    const uint32_t blocks = std::min<uint32_t>((a.rows + wpb - 1) / wpb, 2048u);
    int rc = dispatch_layout(c, [&](auto V, auto E) {
        hipLaunchKernelGGL((push_rows_kernel<decltype(V)::value, decltype(E)::value>), dim3(blocks), dim3(64 * wpb), 0, c->stream, a);
    });
    if (rc != F2V_OK) return rc;
    HIPC(hipGetLastError());
    return F2V_OK;
}

int launch_barrier(f2v_ctx *c);

// End of one exchange: the flag barrier and, in landing-buffer mode, the move of what the peers sent for minibatch
// [lo,hi) (this rank computed [my_lo,my_hi)) from the landing buffer into matrix `which`.
int finish_exchange(f2v_ctx *c, int which, const uint32_t *d_masks, uint32_t lo, uint32_t hi, uint32_t my_lo, uint32_t my_hi) {
    int rc = launch_barrier(c);
    if (rc != F2V_OK) return rc;
    auto &P = c->push;
    if (P.world < 2 || !P.landing) return F2V_OK;
    UnpackArgs u{};
    u.landing = P.landing_buf + (size_t)(P.round & 1u) * P.landing_cap * c->D;
    u.X = c->d_X[which];
    u.masks = d_masks;
    u.lo = lo;
    u.rows = hi - lo;
    u.my_lo = my_lo;
    u.my_hi = my_hi;
    u.D = c->D;
    u.self = P.rank;
    const uint32_t wpb = 4;
    const uint32_t blocks = std::min<uint32_t>((u.rows + wpb - 1) / wpb, 2048u);
    rc = dispatch_layout(c, [&](auto V, auto E) {
        hipLaunchKernelGGL((unpack_rows_kernel<decltype(V)::value, decltype(E)::value>), dim3(blocks), dim3(64 * wpb), 0, c->stream, u);
    });
    if (rc != F2V_OK) return rc;
    HIPC(hipGetLastError());
    P.round++;
    return F2V_OK;
}

int launch_barrier(f2v_ctx *c) {
    if (c->push.world < 2) return F2V_OK;
    BarrierArgs b{};
    b.flags = c->push.flags;
    for (uint32_t r = 0; r < c->push.world; r++) b.peer_flags[r] = c->push.peer_flags[r];
    b.err = c->push.d_err;
    b.seq = ++c->push.seq;
    b.timeout_ticks = ms_to_ticks(c->push.timeout_ms);
    b.self = c->push.rank;
    b.world = c->push.world;
    hipLaunchKernelGGL(xgmi_barrier_kernel, dim3(1), dim3(64), 0, c->stream, b);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// after a stream synchronisation: did every barrier see all peers?
int check_push_err(f2v_ctx *c, const char *where) {
    if (c->push.world < 2) return F2V_OK;
    uint32_t e = 0;
    HIPC(hipMemcpy(&e, c->push.d_err, sizeof e, hipMemcpyDeviceToHost));
    if (e) return fail(F2V_ESTATE, "%s: a peer did not reach the xGMI barrier within %lld ms", where, (long long)c->push.timeout_ms);
    return F2V_OK;
}

int push_detach(f2v_ctx *c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->push.attached && !c->push.local) {
        for (uint32_t r = 0; r < c->push.world; r++) {
            if (r == c->push.rank) continue;
            for (int k = 0; k < 2; k++)
                if (c->push.peer_X[k][r]) (void)hipIpcCloseMemHandle(c->push.peer_X[k][r]);
            if (c->push.peer_flags[r]) (void)hipIpcCloseMemHandle(c->push.peer_flags[r]);
            if (c->push.peer_landing[r]) (void)hipIpcCloseMemHandle(c->push.peer_landing[r]);
        }
    }
    for (int k = 0; k < 2; k++)
        for (int r = 0; r < kMaxRanks; r++) c->push.peer_X[k][r] = nullptr;
    for (int r = 0; r < kMaxRanks; r++) { c->push.peer_flags[r] = nullptr; c->push.peer_landing[r] = nullptr; }
    c->push.attached = false;
    c->push.local = false;
    c->push.rank = 0;
    c->push.world = 1;
    if (c->shared_card) { c->shared_card = false; drop_plans(c); }
    return F2V_OK;
}

// Reader masks of this run in HBM: the neighbour part is static per (batch, world) and cached; the vertices this
// run samples are read by everyone and are patched in (and last run's patched out) by two scatter launches.
int prepare_masks(f2v_ctx *c, uint32_t batch, const std::vector<uint32_t> &ids) {
    auto &P = c->push;
    if (P.mask_batch != batch || P.mask_world != P.world || P.base_masks.size() != c->n || !P.d_masks) {
        P.base_masks.assign(c->n, 0u);
        int rc = f2v_push_masks(c->rowptr.data(), c->colids.data(), c->n, batch, P.world, nullptr, 0, P.base_masks.data());
        if (rc != F2V_OK) return rc;
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(P.d_masks.reserve(c->n, "reader masks"));
        HIPC(hipMemcpy(P.d_masks, P.base_masks.data(), (size_t)c->n * sizeof(uint32_t), hipMemcpyHostToDevice));
        P.patched_ids.clear();
        P.mask_batch = batch;
        P.mask_world = P.world;
        P.pushed_per_epoch = 0;
        for (uint32_t b0 = 0; b0 < c->n; b0 += batch) {
            uint32_t lo, hi;
            shard_of(c, false, b0, (uint32_t)std::min<uint64_t>((uint64_t)b0 + batch, c->n), P.rank, P.world, &lo, &hi);
            for (uint32_t v = lo; v < hi; v++) P.pushed_per_epoch += (uint64_t)__builtin_popcount(P.base_masks[v]);
        }
    }
    // patch list: [restore ids | restore values | set ids | set values]
    std::vector<uint32_t> uniq(ids);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const size_t nr = P.patched_ids.size(), ns = uniq.size();
    if (nr + ns == 0) return F2V_OK;
    std::vector<uint32_t> h(2 * (nr + ns));
    for (size_t k = 0; k < nr; k++) { h[k] = P.patched_ids[k]; h[nr + k] = P.base_masks[P.patched_ids[k]]; }
    const uint32_t everyone = (P.world >= 32 ? 0xFFFFFFFFu : ((1u << P.world) - 1u));
    for (size_t k = 0; k < ns; k++) { h[2 * nr + k] = uniq[k]; h[2 * nr + ns + k] = everyone; }
    HIPC(hipStreamSynchronize(c->stream));
    if (h.size() > P.d_patch.cap) F2VC(P.d_patch.reserve(h.size() * 2, "reader masks"));
    HIPC(hipMemcpy(P.d_patch, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (nr) hipLaunchKernelGGL(mask_patch_kernel, dim3((uint32_t)((nr + 255) / 256)), dim3(256), 0, c->stream, P.d_masks, P.d_patch, P.d_patch + nr, (uint32_t)nr);
    if (ns) hipLaunchKernelGGL(mask_patch_kernel, dim3((uint32_t)((ns + 255) / 256)), dim3(256), 0, c->stream, P.d_masks, P.d_patch + 2 * nr, P.d_patch + 2 * nr + ns, (uint32_t)ns);
    HIPC(hipGetLastError());
    P.patched_ids.swap(uniq);
    return F2V_OK;
}

// ---- parameters (include/f2v.h: f2v_set_param / f2v_get_param) ----------------------------------------------------------------
// before anything the launch plans were built from changes: nothing pending, nothing in flight
int quiesce(f2v_ctx *c) {
    HIPC(hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc != F2V_OK) return rc;
    HIPC(hipStreamSynchronize(c->stream));
    return F2V_OK;
}

enum ParamKind { kValue, kFlag };            // kFlag: a switch -- every value is accepted, non-zero is on
enum Replan { kKeep, kAlways, kOnChange };   // setting it quiesces the handle and drops its launch plans: never, always, where the value changes

struct Param {
    const char *name;
    int64_t (*get)(const f2v_ctx *);       // nullptr: cannot be read
    void (*put)(f2v_ctx *, int64_t);       // stores the value and does nothing else; nullptr (and no `set`): cannot be set
    ParamKind kind = kValue;
    Replan replan = kKeep;
    bool (*valid)(int64_t) = nullptr;      // the accepted values (nullptr: all of them) ...
    const char *error = nullptr;           // ... and what any other one is answered with (F2V_EINVAL)
    int (*set)(f2v_ctx *, int64_t) = nullptr;  // after `valid`: runs instead of the plain rule (`replan` then says what it does)
};

template <int64_t LO, int64_t HI> bool in(int64_t v) { return v >= LO && v <= HI; }
template <int64_t... S> bool one_of(int64_t v) { return ((v == S) || ...); }
bool fanin_ok(int64_t v) { return v == 0 || in<2, 0x7FFFFFFF>(v); }

int set_hub_chunk(f2v_ctx *c, int64_t value) {
    int rc = quiesce(c);
    if (rc != F2V_OK) return rc;
    if (value > (int64_t)kItemSlotMask) return fail(F2V_EINVAL, "hub_chunk out of range");
    // partial-sum slots are 28-bit: pieces plus the nodes of their combine trees must stay below 2^28
    if (value > 0 && c->nnz / (uint64_t)value >= (1ull << 27)) return fail(F2V_EINVAL, "hub_chunk %lld is too small for %llu nonzeros", (long long)value, (unsigned long long)c->nnz);
    c->chunk = (uint32_t)value;
    c->chunk_auto = false;
    drop_plans(c);
    return F2V_OK;
}

int set_hub_chunk_for_batch(f2v_ctx *c, int64_t value) {  // resolve the automatic chunk for this batch size now
    int rc = quiesce(c);
    if (rc != F2V_OK) return rc;
    const uint32_t ch = auto_chunk(c, (uint32_t)value);
    if (ch != c->chunk) { c->chunk = ch; drop_plans(c); }
    c->chunk_auto = true;
    return F2V_OK;
}

int set_nearest_block(f2v_ctx *c, int64_t value) {
    if (value == 128 && c->D > 128) return fail(F2V_EINVAL, "nearest_block = 128 needs dim <= 128 (the query block lives in LDS)");
    c->nn.block = (uint32_t)value;
    return F2V_OK;
}

int set_recover(f2v_ctx *c, int64_t value) {
    c->recover = value != 0;
    if (!c->recover && c->d_snap) {  // the snapshot matrix goes with the net
        HIPC(hipSetDevice(c->device));
        HIPC(hipStreamSynchronize(c->stream));
        c->d_snap.release();
    }
    return F2V_OK;
}

// a row's `get` and `put` where the parameter is one field of the handle
#define F2V_READ(field) [](const f2v_ctx *c) -> int64_t { return (int64_t)c->field; }
#define F2V_GET(field) F2V_READ(field), nullptr
#define F2V_PUT(field) nullptr, [](f2v_ctx *c, int64_t v) { c->field = (decltype(c->field))v; }
#define F2V_FIELD(field) F2V_READ(field), [](f2v_ctx *c, int64_t v) { c->field = (decltype(c->field))v; }
const Param kParams[] = {
    {"hub_chunk", F2V_FIELD(chunk), kValue, kAlways, in<0, 0x7FFFFFFF>, "hub_chunk out of range", set_hub_chunk},
    {"hub_chunk_for_batch", nullptr, nullptr, kValue, kOnChange, in<1, 0xFFFFFFFFll>, "hub_chunk_for_batch: bad batch size", set_hub_chunk_for_batch},
    {"hub_chunk_auto", F2V_GET(chunk_auto)},
    {"hub_fanin", F2V_FIELD(fanin), kValue, kAlways, fanin_ok, "hub_fanin must be 0 (one sequential pass) or >= 2"},
    {"quarter_wave", F2V_FIELD(use_quarter), kFlag, kOnChange},  // the item layout follows the kernel's items per workgroup
    {"waves_per_block", F2V_FIELD(waves_per_block), kValue, kOnChange, one_of<1, 2, 4>, "waves_per_block must be 1, 2 or 4"},
    {"rows_in_flight", F2V_PUT(rows_in_flight), kValue, kKeep, one_of<0, 4, 8>, "rows_in_flight must be 0 (default), 4 or 8"},
    {"fast_rng", F2V_FIELD(fast_rng), kFlag},
    {"use_graph", F2V_FIELD(use_graph), kFlag},
    {"class_cut", F2V_FIELD(class_cut), kFlag, kAlways},
    {"piece_affinity", F2V_FIELD(piece_affinity), kFlag, kOnChange},
    {"count_compulsory", F2V_FIELD(count_compulsory), kFlag, kOnChange},
    {"shared_card", F2V_GET(shared_card)},
    {"merge_finalize", F2V_READ(merge_fin), [](f2v_ctx *c, int64_t v) { c->merge_fin = v != 0; c->waits_suspended = false; /* the caller's own choice stands */ }, kFlag},
    {"tree_timeout_ms", F2V_FIELD(tree_timeout_ms), kValue, kKeep, in<1, 600000>, "tree_timeout_ms must be 1..600000"},
    {"chain_timeout_ms", F2V_FIELD(chain_timeout_ms), kValue, kKeep, in<1, 600000>, "chain_timeout_ms must be 1..600000"},
    {"recover", F2V_FIELD(recover), kFlag, kKeep, nullptr, nullptr, set_recover},
    {"recoveries", F2V_GET(recoveries)},
    {"chain_batches", F2V_FIELD(chain), kFlag},
    {"chain_max_batch", F2V_FIELD(chain_max_batch), kValue, kKeep, in<0, 0xFFFFFFFFll>, "chain_max_batch out of range"},
    // rows one chained launch covers: an explicit value holds for both forms ("wide_rows" alone: the wide form's)
    {"chain_rows", F2V_READ(chain_rows), [](f2v_ctx *c, int64_t v) { c->chain_rows = c->wide_rows = (uint32_t)v; }, kValue, kAlways, in<2, 0x7FFFFFFF>, "chain_rows out of range"},
    {"chain_wide", F2V_FIELD(wide), kFlag, kAlways},
    {"wide_rows", F2V_FIELD(wide_rows), kValue, kAlways, in<2, 0x7FFFFFFF>, "wide_rows out of range"},
    {"wide_max_batch", F2V_FIELD(wide_max_batch), kValue, kKeep, in<0, 0xFFFFFFFFll>, "wide_max_batch out of range"},
    {"wide_min_width", F2V_FIELD(wide_min_width), kValue, kAlways, one_of<0, 16, 32, 64, 128>, "wide_min_width must be 0 (automatic), 16, 32, 64 or 128"},
    {"wide_phases", F2V_FIELD(wide_phases), kValue, kAlways, in<1, 64>, "wide_phases must be 1..64"},
    {"wide_span", F2V_FIELD(wide_span), kValue, kAlways, in<1, 64>, "wide_span must be 1..64"},
    {"wide_finish", F2V_FIELD(wide_finish), kValue, kAlways, in<1, 64>, "wide_finish must be 1..64"},
    {"wide_order", F2V_FIELD(wide_order), kValue, kAlways, in<0, 2>, "wide_order must be 0, 1 or 2"},
    {"wide_rounds", F2V_FIELD(wide_rounds), kValue, kAlways, in<0, 64>, "wide_rounds must be 0..64"},
    {"wide_epochs", F2V_FIELD(wide_epochs), kValue, kKeep, in<0, 1024>, "wide_epochs must be 0 (automatic) ... 1024"},
    {"wide_single", F2V_FIELD(wide_single), kFlag},
    {"wide_samples_early", F2V_FIELD(wide_samples_early), kValue, kKeep, in<-1, 1>, "wide_samples_early must be -1 (automatic), 0 or 1"},
    {"replicate_small", F2V_FIELD(replicate_small), kValue, kKeep, in<0, 2>, "replicate_small must be 0 (never), 1 (where no peer shares the GPU) or 2 (always)"},
    {"epoch_marks", F2V_FIELD(mark_every), kValue, kKeep, in<0, 0x7FFFFFFF>, "epoch_marks out of range"},
    {"loss_every", F2V_FIELD(loss_every), kValue, kKeep, in<0, 0x7FFFFFFF>, "loss_every out of range"},
    {"loss_seed", F2V_FIELD(loss_seed)},
    {"last_loss_us", [](const f2v_ctx *c) { return (int64_t)(c->last_loss_us + 0.5); }, nullptr},
    // candidate ranges a query block's work is cut into (0: chosen from nq and N); results do not depend on it
    {"nearest_splits", F2V_FIELD(nn.splits), kValue, kKeep, in<0, 256>, "nearest_splits must be 0..256"},
    // queries per workgroup (0: 128 where D <= 128 and more than 32 queries share a launch, else 32)
    {"nearest_block", F2V_FIELD(nn.block), kValue, kKeep, one_of<0, 32, 128>, "nearest_block must be 0, 32 or 128", set_nearest_block},
    // queries per launch: bounds the workspace (chunk x splits x k keys)
    {"nearest_chunk", F2V_FIELD(nn.chunk), kValue, kKeep, in<1, 65536>, "nearest_chunk must be 1..65536"},
    // queries per launch of an index search: bounds its workspace (chunk x probes x ranges x k keys); results do not depend on it
    {"index_chunk", F2V_FIELD(ix.chunk), kValue, kKeep, in<1, 65536>, "index_chunk must be 1..65536"},
    // tiles of 128 candidates per work item of the index scan (longer lists are cut into ranges); results do not depend on it
    {"index_split_tiles", F2V_FIELD(ix.split_tiles), kValue, kKeep, in<1, 65536>, "index_split_tiles must be 1..65536"},
    // queries per work item of the index scan (0: 128 where D <= 128 and a bucket has more than 32 queries left, else 32); results do not depend on it
    {"index_block", F2V_FIELD(ix.block), kValue, kKeep, one_of<0, 32>, "index_block must be 0 or 32"},
    // rows per workgroup of the k-means assignment kernel (0: 256 for k <= 2, 128 for k <= 4, else 64); results do not depend on it
    {"kmeans_block", F2V_FIELD(km.block), kValue, kKeep, one_of<0, 64, 128, 256>, "kmeans_block must be 0, 64, 128 or 256"},
    // samples per launch of the silhouette: bounds its workspace (chunk x spans doubles); results do not depend on it
    {"separation_chunk", F2V_FIELD(sep.chunk), kValue, kKeep, in<1, 1048576>, "separation_chunk must be 1..1048576"},
    // sample rows per workgroup of separation_pair_kernel (0: 64); results do not depend on it
    {"separation_block", F2V_FIELD(sep.block), kValue, kKeep, one_of<0, 64, 128>, "separation_block must be 0, 64 or 128"},
    // samples per launch of the trustworthiness kernels: bounds their workspace (chunk x k keys and counts); results do not depend on it
    {"trust_chunk", F2V_FIELD(lay.chunk), kValue, kKeep, in<1, 1048576>, "trust_chunk must be 1..1048576"},
    // sample rows per workgroup of trust_rank_kernel (0: 64; 128 holds where k <= 32, its thresholds live in LDS); results do not depend on it
    {"trust_block", F2V_FIELD(lay.block), kValue, kKeep, one_of<0, 64, 128>, "trust_block must be 0, 64 or 128"},
    // rows per workgroup of tsne_pair_kernel (0: 64 below 4096 points, else 256) and spans per workgroup of it (0: one); results do
    // not depend on them
    {"tsne_rows", F2V_FIELD(ts.rows), kValue, kKeep, one_of<0, 64, 128, 256>, "tsne_rows must be 0 (automatic), 64, 128 or 256"},
    {"tsne_slices", F2V_FIELD(ts.slices), kValue, kKeep, in<0, 65536>, "tsne_slices must be 0 (automatic) ... 65536"},
    // rows per workgroup of exact_pair_kernel (0: from the minibatch and the spans, so that the grid fills the card); results do not depend on it
    {"exact_rows", F2V_FIELD(ex.rows), kValue, kKeep, one_of<0, 4, 8, 16>, "exact_rows must be 0 (automatic), 4, 8 or 16"},
    // fewest rows of a minibatch that run the quarter-wave pair kernel where D allows it (0: every minibatch); results do not depend on it
    {"exact_quarter_min", F2V_FIELD(ex.quarter_min), kValue, kKeep, in<0, 0xFFFFFFFFll>, "exact_quarter_min out of range"},
    // what the last minibatch of the last f2v_train(option 1) ran with: rows per workgroup, and whether the quarter-wave kernel
    {"last_exact_rows", F2V_GET(ex.last_rows)},
    {"last_exact_quarter", F2V_GET(ex.last_quarter)},
    // the index e of the first epoch of the next f2v_train(option 1): STEP_e; a call of `iters` epochs advances it by `iters`
    {"exact_epoch", F2V_FIELD(ex.epoch), kValue, kKeep, in<0, 0x7FFFFFFF>, "exact_epoch must be 0..2^31-1"},
    // new vertices per launch of f2v_fold_in: bounds its workspace (two chunk x D matrices); results do not depend on it
    {"fold_chunk", F2V_FIELD(fold.chunk), kValue, kKeep, in<1, 1048576>, "fold_chunk must be 1..1048576"},
    // f2v_fold_in: 0 = every epoch gathers a vertex's list rows from the caches, -1 = automatic (the same); 1, rows staged in LDS once, was measured slower and is not built
    {"fold_resident", F2V_FIELD(fold.resident), kValue, kKeep, in<-1, 0>, "fold_resident must be -1 (automatic) or 0: the resident form measured slower and is not part of this build"},
    // f2v_link_pairs: a vertex with at most this many negatives is one wavefront's (its accepted set a list in LDS), a longer one a workgroup's (a table); placement only
    {"link_short_max", F2V_FIELD(link.short_max), kValue, kKeep, in<0, kLinkShortLimit>, "link_short_max must be 0..1024"},
    // f2v_pair_scores: pairs per upload and launch: bounds its workspace (12 bytes a pair); results do not depend on it
    {"pairs_chunk", F2V_FIELD(held.pairs_chunk), kValue, kKeep, in<1, 1 << 26>, "pairs_chunk must be 1..67108864"},
    // f2v_pair_neighbourhood: 1 = the pieces of a pair whose S row has several are work items of their own, 0 = one wavefront walks them; placement only
    {"neighbourhood_spread", F2V_FIELD(nb.spread), kFlag},
    {"last_neighbourhood_items", F2V_GET(nb.last_items)},
    // f2v_pair_ranks: pairs per launch: bounds its workspace (chunk x D floats and 20 bytes a pair); results do not depend on it
    {"ranks_chunk", F2V_FIELD(pr.chunk), kValue, kKeep, in<1, 65536>, "ranks_chunk must be 1..65536"},
    // candidate ranges a query block's counting is cut into (0: chosen from the query blocks and the tiles); results do not depend on it
    {"ranks_splits", F2V_FIELD(pr.splits), kValue, kKeep, in<0, 256>, "ranks_splits must be 0..256"},
    // device time of the last f2v_pair_ranks' base-count launches and of its correction launches
    {"last_ranks_base_us", [](const f2v_ctx *c) { return (int64_t)(c->pr.base_seconds * 1e6 + 0.5); }, nullptr},
    {"last_ranks_correct_us", [](const f2v_ctx *c) { return (int64_t)(c->pr.correct_seconds * 1e6 + 0.5); }, nullptr},
    // f2v_louvain: a unit whose rows hold at most this many nonzeros is gathered by 16 lanes (table in LDS), a longer one by a workgroup; placement only
    {"louvain_short_max", F2V_FIELD(lv.short_max), kValue, kKeep, in<0, kLouvainShortLimit>, "louvain_short_max must be 0..256"},
    // f2v_louvain: the largest table (slots) a workgroup keeps in LDS; a longer one lies in the workspace; placement only
    {"louvain_lds_slots", F2V_FIELD(lv.lds_slots), kValue, kKeep, in<0, kLouvainLdsLimit>, "louvain_lds_slots must be 0..8192"},
    // f2v_spanning_forest, f2v_edge_split_connected: the forest's order compares the leading `bits` bits of a key, then (a, b).  A
    // diagnostic knob: small values force key ties so that the tie-break runs; it never affects which pairs are hold-out candidates
    {"last_subgraph_us", [](const f2v_ctx *c) { return (int64_t)(c->cc_subgraph_seconds * 1e6 + 0.5); }, nullptr},
    {"forest_key_bits", F2V_FIELD(cc.key_bits), kValue, kKeep, in<1, 64>, "forest_key_bits must be 1..64"},
    {"push_fused", F2V_FIELD(push.fused), kFlag},
    {"push_timeout_ms", F2V_FIELD(push.timeout_ms), kValue, kKeep, in<1, 600000>, "push_timeout_ms must be 1..600000"},
    // takes effect at the next f2v_push_export; read: what the exchange in place runs with
    {"push_landing", [](const f2v_ctx *c) -> int64_t { return (c->push.attached || c->push.exported) ? c->push.landing : c->push.force_landing; },
     [](f2v_ctx *c, int64_t v) { c->push.force_landing = v != 0; }, kFlag},
    {"push_world", [](const f2v_ctx *c) -> int64_t { return c->push.attached ? c->push.world : 0; }, nullptr},
    {"push_rank", F2V_GET(push.rank)},
    {"last_train_replicated", F2V_GET(last_replicated)},
    {"last_train_form", F2V_GET(last_train_form)},
    {"last_wide_width", F2V_GET(last_wide_width)},
    {"last_wide_early", F2V_GET(last_wide_early)},
    {"last_wide_epochs", F2V_GET(last_wide_epochs)},
    // launch plans resident on the host (and, uploaded, in HBM): items, jobs, workgroup descriptors, tree nodes
    {"plan_resident_bytes", [](const f2v_ctx *c) { return (int64_t)(c->plan_items.bytes() + c->plan_jobs.bytes() + c->plan_wide.bytes() + c->plan_wg.bytes() + c->plan_hubs.bytes()); }, nullptr},
    {"xcc_count", F2V_GET(xcc_count)},
    {"xcc_round_robin", F2V_GET(xcc_round_robin)},
    {"dim", F2V_GET(D)},
    {"n", F2V_GET(n)},
    {"nnz", F2V_GET(nnz)},
};
#undef F2V_READ
#undef F2V_GET
#undef F2V_PUT
#undef F2V_FIELD

const Param *find_param(const char *name) {
    for (const Param &p : kParams)
        if (!strcmp(p.name, name)) return &p;
    return nullptr;
}

int train_impl(f2v_ctx *c, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode, double *seconds_out, bool sharded);
int train_exact(f2v_ctx *c, uint32_t iters, uint32_t batch, int bs_mode, double *seconds_out);
int launch_exact_objective(f2v_ctx *c, const float *X, ObjPartial *out);
int exact_objective_prepare(f2v_ctx *c);

}  // namespace

extern "C" {

int f2v_create(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint64_t nnz, uint32_t dim, int device,
               f2v_handle *out) {
    if (!rowptr || (!colids && nnz) || !out) return fail(F2V_EINVAL, "f2v_create: null argument");
    if (n < 2) return fail(F2V_EINVAL, "f2v_create: need at least 2 vertices (rand() %% (N-1))");
    if (dim == 0 || dim > 512) return fail(F2V_EINVAL, "f2v_create: dim %u outside 1..512", dim);
    if (nnz >= 0xFFFFFFFFull) return fail(F2V_EINVAL, "f2v_create: nnz exceeds 32-bit row pointers");
    if (rowptr[0] != 0 || rowptr[n] != nnz) return fail(F2V_EINVAL, "f2v_create: rowptr[0] must be 0 and rowptr[n] == nnz");
    for (uint32_t i = 0; i < n; i++)
        if (rowptr[i + 1] < rowptr[i]) return fail(F2V_EINVAL, "f2v_create: rowptr not monotone at row %u", i);
    for (uint64_t k = 0; k < nnz; k++)
        if (colids[k] >= n) return fail(F2V_EINVAL, "f2v_create: colids[%llu] = %u is not a vertex", (unsigned long long)k, colids[k]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(F2V_ENODEV, "f2v_create: no HIP device visible (libf2v has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(F2V_ENODEV, "f2v_create: device %d not in [0,%d)", device, ndev);
    HIPC(hipSetDevice(device));
    f2v_ctx *c = new f2v_ctx();
    c->device = device;
    c->n = n;
    c->nnz = nnz;
    c->D = dim;
    c->vec = pick_vec(dim);
    c->exact = ((uint32_t)(64 * c->vec) == dim);
    c->rowptr.assign(rowptr, rowptr + n + 1);
    c->colids.assign(colids, colids + nnz);
    c->rng.seed(1);
    auto bail = [&](int rc) { f2v_destroy(c); return rc; };
#define HIPB(expr)                                                                                                   \
    do {                                                                                                             \
        hipError_t e__ = (expr);                                                                                     \
        if (e__ != hipSuccess)                                                                                       \
            return bail(fail(e__ == hipErrorOutOfMemory ? F2V_ENOMEM : F2V_ENODEV, "%s: %s", #expr, hipGetErrorString(e__))); \
    } while (0)
#define F2VB(expr)                              \
    do {                                        \
        int rc__ = (expr);                      \
        if (rc__ != F2V_OK) return bail(rc__);  \
    } while (0)
    HIPB(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    F2VB(c->d_rowptr.reserve((size_t)n + 1, "graph"));
    F2VB(c->d_colids.reserve(nnz, "graph"));
    for (int k = 0; k < 2; k++) F2VB(c->d_X[k].reserve(((size_t)n + kPadRows) * dim, "embedding"));
    F2VB(c->d_table.reserve(kSmTableSize, "sigmoid table"));
    F2VB(c->d_kerr.reserve(16, "kernel error words"));
    HIPB(hipMemsetAsync(c->d_kerr, 0, 64, c->stream));
    HIPB(hipStreamSynchronize(c->stream));
    HIPB(hipMemcpy(c->d_rowptr, rowptr, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (nnz) HIPB(hipMemcpy(c->d_colids, colids, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    float table[kSmTableSize];
    sm_table_host(table);
    HIPB(hipMemcpy(c->d_table, table, sizeof table, hipMemcpyHostToDevice));
    F2VB(c->h_kerr.reserve(4 * 16));
    memset(c->h_kerr, 0, 4 * 64);
    if (const char *e = getenv("F2V_TREE_TIMEOUT_MS")) {
        const long ms = atol(e);
        if (ms > 0 && ms <= 600000) c->tree_timeout_ms = ms;
    }
    if (const char *e = getenv("F2V_RECOVER")) c->recover = atoi(e) != 0;  // default of "recover" for new handles
#ifdef F2V_TEST_HOOKS
    if (const char *e = getenv("F2V_TEST_WITHHOLD_SLOT")) c->hooks.withhold_slot = (uint32_t)strtoul(e, nullptr, 0);  // f2v_test_withhold_flag from outside
    if (const char *e = getenv("F2V_TEST_WITHHOLD_ROW")) c->hooks.withhold_row = (uint32_t)strtoul(e, nullptr, 0);
#endif
    {
        // Dispatch probe: the one-launch minibatch (combine-tree nodes waiting inside the step kernel's grid) counts on
        // 8 XCDs taking workgroups round robin.  Checked here, on this device as this process sees it; if it does not
        // hold the handle starts with "merge_finalize" = 0 (one launch per tree level: no in-grid waits at all).
        constexpr uint32_t kProbe = 256;
        DevBuf<uint32_t> d_x;
        uint32_t h_x[kProbe];
        F2VB(d_x.reserve(kProbe, "dispatch probe"));
        hipLaunchKernelGGL(xcc_probe_kernel, dim3(kProbe), dim3(64), 0, c->stream, d_x);
        HIPB(hipGetLastError());
        HIPB(hipMemcpyAsync(h_x, d_x, sizeof h_x, hipMemcpyDeviceToHost, c->stream));
        HIPB(hipStreamSynchronize(c->stream));
        uint32_t seen = 0;
        bool rr = true;
        for (uint32_t b = 0; b < kProbe; b++) {
            seen |= 1u << (h_x[b] & 15u);
            if (h_x[b] != h_x[b % 8u]) rr = false;
        }
        c->xcc_count = (uint32_t)__builtin_popcount(seen);
        for (uint32_t b = 1; b < 8u; b++)
            for (uint32_t k = 0; k < b; k++)
                if (h_x[b] == h_x[k]) rr = false;
        c->xcc_round_robin = rr && c->xcc_count == 8u;
        if (!c->xcc_round_robin) c->merge_fin = false;
    }
#undef F2VB
#undef HIPB
    *out = c;
    return F2V_OK;
}

int f2v_destroy(f2v_handle c) {
    if (!c) return F2V_OK;
    (void)hipSetDevice(c->device);
    (void)push_detach(c);  // the peers' IPC mappings are closed before anything is freed
    const hipStream_t stream = c->stream;
    delete c;  // every buffer, pinned array and event of the handle owns itself and goes with it: before their stream
    if (stream) (void)hipStreamDestroy(stream);
    return F2V_OK;
}

int f2v_srand(f2v_handle c, uint32_t seed) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    c->rng.seed(seed);
    c->fast_seed = seed;
    c->fast_epoch = 0;
    return F2V_OK;
}

int f2v_rand_index(f2v_handle c, uint32_t max_num, uint32_t min_num, uint32_t *out) {
    if (!c || !out || max_num <= min_num) return fail(F2V_EINVAL, "f2v_rand_index: bad argument");
    *out = c->rng.index(max_num, min_num);
    return F2V_OK;
}

int f2v_rand_indices(f2v_handle c, uint32_t max_num, uint32_t min_num, uint64_t count, uint64_t keep, uint32_t *out) {
    if (!c || max_num <= min_num || keep > count || (keep && !out)) return fail(F2V_EINVAL, "f2v_rand_indices: bad argument");
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t r = c->rng.index(max_num, min_num);
        if (k < keep) out[k] = r;
    }
    return F2V_OK;
}

int f2v_init_embeddings(f2v_handle c, int kind) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (kind != F2V_INIT_SYMMETRIC && kind != F2V_INIT_UNIT) return fail(F2V_EINVAL, "f2v_init_embeddings: kind %d", kind);
    HIPC(hipSetDevice(c->device));
    const size_t total = (size_t)c->n * c->D;
    if (c->fast_rng) {  // non-parity: hash-based uniform values generated in HBM
        HIPC(hipStreamSynchronize(c->stream));
        c->pending = false;
        c->upd_lo = c->upd_hi = 0;
        hipLaunchKernelGGL(fast_init_kernel, dim3(4096), dim3(256), 0, c->stream, c->d_X[c->cur], (uint64_t)total, kind, c->fast_seed * 0x9E3779B97F4A7C15ull + 17);
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(c->stream));
        c->have_x = true;
        c->x_invalid = false;
        return F2V_OK;
    }
    HIPC(hipStreamSynchronize(c->stream));
    c->pending = false;
    c->upd_lo = c->upd_hi = 0;
    constexpr size_t kPiece = (size_t)64 << 20;  // floats: 256 MiB
    if (total >= 2 * kPiece) {
        // Large matrices (8 GiB at RMAT-24): the one serial rand() stream is filled piece by piece into two pinned staging
        // buffers by the fill threads (jump-ahead states, bit-identical to the serial stream) while the previous piece
        // travels to HBM -- the pageable-memory copy of the whole matrix used to take longer than generating it.
        HostBuf<float> stage[2];
        DevEvents events;
        hipEvent_t done[2];
        bool used[2] = {false, false};
        for (int k = 0; k < 2; k++) {
            F2VC(stage[k].reserve(kPiece));
            F2VC(events.make(&done[k], hipEventDisableTiming));
        }
        int k = 0;
        for (size_t off = 0; off < total; off += kPiece, k ^= 1) {
            const size_t len = std::min(kPiece, total - off);
            if (used[k]) HIPC(hipEventSynchronize(done[k]));
            init_embeddings_host(c->rng, stage[k], len, kind);
            HIPC(hipMemcpyAsync(c->d_X[c->cur] + off, stage[k], len * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPC(hipEventRecord(done[k], c->stream));
            used[k] = true;
        }
        HIPC(hipStreamSynchronize(c->stream));
    } else {
        std::unique_ptr<float[]> x(new float[total]);  // not value-initialised: the fill threads are the first to touch it
        init_embeddings_host(c->rng, x.get(), total, kind);
        HIPC(hipMemcpy(c->d_X[c->cur], x.get(), total * sizeof(float), hipMemcpyHostToDevice));
    }
    c->have_x = true;
    c->x_invalid = false;
    return F2V_OK;
}

int f2v_set_embeddings(f2v_handle c, const float *x) {
    if (!c || !x) return fail(F2V_EINVAL, "f2v_set_embeddings: null argument");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    c->pending = false;
    c->upd_lo = c->upd_hi = 0;
    HIPC(hipMemcpy(c->d_X[c->cur], x, (size_t)c->n * c->D * sizeof(float), hipMemcpyHostToDevice));
    c->have_x = true;
    c->x_invalid = false;
    return F2V_OK;
}

int f2v_get_embeddings(f2v_handle c, float *x_out) {
    if (!c || !x_out) return fail(F2V_EINVAL, "f2v_get_embeddings: null argument");
    int rc = settled_enter(c, "f2v_get_embeddings");
    if (rc != F2V_OK) return rc;
    HIPC(hipStreamSynchronize(c->stream));
    if ((rc = check_kernel_err(c, "f2v_get_embeddings")) != F2V_OK) return rc;
    HIPC(hipMemcpy(x_out, c->d_X[c->cur], (size_t)c->n * c->D * sizeof(float), hipMemcpyDeviceToHost));
    return F2V_OK;
}

int f2v_set_param(f2v_handle c, const char *name, int64_t value) {
    if (!c || !name) return fail(F2V_EINVAL, "f2v_set_param: null argument");
    const Param *p = find_param(name);
    if (!p || (!p->put && !p->set)) return fail(F2V_EINVAL, "f2v_set_param: unknown parameter '%s'", name);
    if (p->valid && !p->valid(value)) return fail(F2V_EINVAL, "%s", p->error);
    if (p->kind == kFlag) value = value != 0;
    if (p->set) return p->set(c, value);
    if (p->replan == kAlways || (p->replan == kOnChange && p->get(c) != value)) {
        int rc = quiesce(c);
        if (rc != F2V_OK) return rc;
        p->put(c, value);
        drop_plans(c);
    } else {
        p->put(c, value);
    }
    return F2V_OK;
}

int f2v_get_param(f2v_handle c, const char *name, int64_t *out) {
    if (!c || !name || !out) return fail(F2V_EINVAL, "f2v_get_param: null argument");
    const Param *p = find_param(name);
    if (!p || !p->get) return fail(F2V_EINVAL, "f2v_get_param: unknown parameter '%s'", name);
    *out = p->get(c);
    return F2V_OK;
}

int f2v_set_walks(f2v_handle c, const uint32_t *walks) {
    if (!c || !walks) return fail(F2V_EINVAL, "f2v_set_walks: null argument");
    HIPC(hipSetDevice(c->device));
    const size_t cnt = (size_t)c->n * kWalkLength;
    for (size_t k = 0; k < cnt; k++)
        if (walks[k] >= c->n) return fail(F2V_EINVAL, "f2v_set_walks: walks[%zu] = %u is not a vertex", k, walks[k]);
    F2VC(current_walks(c));
    // stream-ordered after every step that still reads the previous epoch's walks
    HIPC(hipMemcpyAsync(c->d_walks, walks, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    c->have_walks = true;
    return F2V_OK;
}

// non-parity walks generated in HBM (see fast_walks_kernel)
static int fast_walks(f2v_ctx *c) {
    F2VC(current_walks(c));
    hipLaunchKernelGGL(fast_walks_kernel, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->d_rowptr, c->d_colids, c->n, c->nnz,
                       c->d_walks, c->fast_seed * 0xD1342543DE82EF95ull + 5, c->fast_epoch++);
    HIPC(hipGetLastError());
    c->have_walks = true;
    return F2V_OK;
}

int f2v_generate_walks(f2v_handle c, uint32_t *walks_out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (c->fast_rng) {
        HIPC(hipSetDevice(c->device));
        int rc = fast_walks(c);
        if (rc != F2V_OK) return rc;
        if (walks_out) {
            HIPC(hipStreamSynchronize(c->stream));
            HIPC(hipMemcpy(walks_out, c->d_walks, (size_t)c->n * kWalkLength * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        return F2V_OK;
    }
    std::vector<uint32_t> w;
    generate_walks_host(c, w);
    if (walks_out) memcpy(walks_out, w.data(), w.size() * sizeof(uint32_t));
    return f2v_set_walks(c, w.data());
}

int f2v_minibatch_step(f2v_handle c, int option, uint32_t batch_lo, uint32_t batch_hi, uint32_t row_lo,
                       uint32_t row_hi, const uint32_t *sample_ids, uint32_t n_sample_ids, uint32_t ns, float lr,
                       int bs_mode) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (option == 1) return fail(F2V_EINVAL, "f2v_minibatch_step: option 1 (exact all-pairs Force2Vec) runs on a single GPU, f2v_train only");
    const int math = math_of_option(option);
    if (!math) return fail(F2V_EINVAL, "f2v_minibatch_step: option %d is outside 5..11", option);
    c->unit_degi = option == 10;
    if (!c->have_x) return fail(F2V_ESTATE, "f2v_minibatch_step: embeddings not initialised");
    if (batch_lo >= batch_hi || batch_hi > c->n) return fail(F2V_EINVAL, "f2v_minibatch_step: bad batch [%u,%u)", batch_lo, batch_hi);
    if (row_lo < batch_lo || row_hi > batch_hi || row_lo > row_hi) return fail(F2V_EINVAL, "f2v_minibatch_step: rows [%u,%u) outside the batch", row_lo, row_hi);
    if (math == 7 && bs_mode) return fail(F2V_EINVAL, "option 7 has no -bs 1 variant");
    if (math == 7 && !c->have_walks) return fail(F2V_ESTATE, "option 7 needs f2v_set_walks / f2v_generate_walks first");
    const uint32_t need = bs_mode ? (batch_hi - batch_lo) + ns - 1 : ns;
    if (ns && (!sample_ids || n_sample_ids < need)) return fail(F2V_EINVAL, "f2v_minibatch_step: %u sample ids needed, %u given", need, n_sample_ids);
    for (uint32_t k = 0; k < need; k++)
        if (sample_ids[k] >= c->n) return fail(F2V_EINVAL, "f2v_minibatch_step: sample id %u is not a vertex", sample_ids[k]);
    HIPC(hipSetDevice(c->device));
    int rc = c->d_ids.reserve(c, std::max<size_t>(need, 64), "sample ids");
    if (rc != F2V_OK) return rc;
    // the previous step may still be reading d_ids: order the copy behind it on the stream
    c->ids_valid = 0;
    if (need) {
        HIPC(hipMemcpyAsync(c->d_ids, sample_ids, need * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    return launch_step(c, math, batch_lo, batch_hi, row_lo, row_hi, c->d_ids, ns, lr, bs_mode);
}

int f2v_upload_sample_ids(f2v_handle c, const uint32_t *ids, uint64_t count) {
    if (!c || (!ids && count)) return fail(F2V_EINVAL, "f2v_upload_sample_ids: null argument");
    for (uint64_t k = 0; k < count; k++)
        if (ids[k] >= c->n) return fail(F2V_EINVAL, "f2v_upload_sample_ids: id %u is not a vertex", ids[k]);
    HIPC(hipSetDevice(c->device));
    int rc = c->d_ids.reserve(c, std::max<size_t>(count, 64), "sample ids");
    if (rc != F2V_OK) return rc;
    HIPC(hipStreamSynchronize(c->stream));  // steps in flight still read the previous ids
    if (count) HIPC(hipMemcpy(c->d_ids, ids, count * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->ids_valid = count;
    return F2V_OK;
}

int f2v_minibatch_step_at(f2v_handle c, int option, uint32_t batch_lo, uint32_t batch_hi, uint32_t row_lo,
                          uint32_t row_hi, uint64_t ids_offset, uint32_t ns, float lr, int bs_mode) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (option == 1) return fail(F2V_EINVAL, "f2v_minibatch_step_at: option 1 (exact all-pairs Force2Vec) runs on a single GPU, f2v_train only");
    const int math = math_of_option(option);
    if (!math) return fail(F2V_EINVAL, "f2v_minibatch_step_at: option %d is outside 5..11", option);
    c->unit_degi = option == 10;
    if (!c->have_x) return fail(F2V_ESTATE, "f2v_minibatch_step_at: embeddings not initialised");
    if (batch_lo >= batch_hi || batch_hi > c->n) return fail(F2V_EINVAL, "f2v_minibatch_step_at: bad batch [%u,%u)", batch_lo, batch_hi);
    if (row_lo < batch_lo || row_hi > batch_hi || row_lo > row_hi) return fail(F2V_EINVAL, "f2v_minibatch_step_at: rows [%u,%u) outside the batch", row_lo, row_hi);
    if (math == 7 && bs_mode) return fail(F2V_EINVAL, "option 7 has no -bs 1 variant");
    if (math == 7 && !c->have_walks) return fail(F2V_ESTATE, "option 7 needs f2v_set_walks / f2v_generate_walks first");
    const uint64_t need = bs_mode ? (uint64_t)(batch_hi - batch_lo) + ns - 1 : ns;
    if (ids_offset + need > c->ids_valid) return fail(F2V_EINVAL, "f2v_minibatch_step_at: ids [%llu,+%llu) were not uploaded", (unsigned long long)ids_offset, (unsigned long long)need);
    HIPC(hipSetDevice(c->device));
    return launch_step(c, math, batch_lo, batch_hi, row_lo, row_hi, c->d_ids + ids_offset, ns, lr, bs_mode);
}

int f2v_flush(f2v_handle c) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    int rc = quiesce(c);
    return rc != F2V_OK ? rc : check_kernel_err(c, "f2v_flush");
}

int f2v_synchronize(f2v_handle c) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    return F2V_OK;
}

int f2v_stage_reserve(f2v_handle c, uint32_t rows) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    // new rows are written in place into the second matrix, which has kPadRows of slack behind row N
    if (rows > c->n + kPadRows) return fail(F2V_EINVAL, "f2v_stage_reserve: %u rows exceed the matrix", rows);
    return F2V_OK;
}

int f2v_stage_device_ptr(f2v_handle c, uint64_t *devptr_out, uint32_t *cap_out) {
    if (!c || !devptr_out) return fail(F2V_EINVAL, "f2v_stage_device_ptr: null argument");
    if (!c->pending) return fail(F2V_ESTATE, "f2v_stage_device_ptr: no minibatch is pending");
    *devptr_out = (uint64_t)(uintptr_t)(c->d_X[c->cur ^ 1] + (size_t)c->p_lo * c->D);
    if (cap_out) *cap_out = c->n + kPadRows - c->p_lo;
    return F2V_OK;
}

int f2v_stage_read(f2v_handle c, uint32_t row_lo, uint32_t row_hi, float *out) {
    if (!c || !out) return fail(F2V_EINVAL, "f2v_stage_read: null argument");
    if (!c->pending || row_lo < c->p_lo || row_hi > c->p_hi || row_lo > row_hi) return fail(F2V_ESTATE, "f2v_stage_read: rows outside the pending minibatch");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(out, c->d_X[c->cur ^ 1] + (size_t)row_lo * c->D, (size_t)(row_hi - row_lo) * c->D * sizeof(float), hipMemcpyDeviceToHost));
    return F2V_OK;
}

int f2v_stage_write(f2v_handle c, uint32_t row_lo, uint32_t row_hi, const float *in) {
    if (!c || !in) return fail(F2V_EINVAL, "f2v_stage_write: null argument");
    if (!c->pending || row_lo < c->p_lo || row_hi > c->p_hi || row_lo > row_hi) return fail(F2V_ESTATE, "f2v_stage_write: rows outside the pending minibatch");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(c->d_X[c->cur ^ 1] + (size_t)row_lo * c->D, in, (size_t)(row_hi - row_lo) * c->D * sizeof(float), hipMemcpyHostToDevice));
    return F2V_OK;
}

int f2v_rows_read(f2v_handle c, const uint32_t *ids, uint32_t count, float *out) {
    if (!c || (count && (!ids || !out))) return fail(F2V_EINVAL, "f2v_rows_read: null argument");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    const float *base = c->d_X[c->cur ^ 1];
    for (uint32_t k = 0; k < count; k++) {
        if (ids[k] >= c->n) return fail(F2V_EINVAL, "f2v_rows_read: id %u is not a vertex", ids[k]);
        HIPC(hipMemcpy(out + (size_t)k * c->D, base + (size_t)ids[k] * c->D, (size_t)c->D * sizeof(float), hipMemcpyDeviceToHost));
    }
    return F2V_OK;
}

int f2v_rows_write(f2v_handle c, const uint32_t *ids, uint32_t count, const float *in) {
    if (!c || (count && (!ids || !in))) return fail(F2V_EINVAL, "f2v_rows_write: null argument");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    float *base = c->d_X[c->cur ^ 1];
    for (uint32_t k = 0; k < count; k++) {
        if (ids[k] >= c->n) return fail(F2V_EINVAL, "f2v_rows_write: id %u is not a vertex", ids[k]);
        HIPC(hipMemcpy(base + (size_t)ids[k] * c->D, in + (size_t)k * c->D, (size_t)c->D * sizeof(float), hipMemcpyHostToDevice));
    }
    return F2V_OK;
}

int f2v_embeddings_device_ptr(f2v_handle c, uint64_t *out) {
    if (!c || !out) return fail(F2V_EINVAL, "null argument");
    *out = (uint64_t)(uintptr_t)c->d_X[c->cur].p;  // the whole matrix only after f2v_flush
    return F2V_OK;
}

int f2v_stream(f2v_handle c, uint64_t *out) {
    if (!c || !out) return fail(F2V_EINVAL, "null argument");
    *out = (uint64_t)(uintptr_t)c->stream;
    return F2V_OK;
}

int f2v_get_stats(f2v_handle c, f2v_stats *out) {
    if (!c || !out) return fail(F2V_EINVAL, "null argument");
    *out = c->stats;
    out->recoveries = c->recoveries;
    out->merge_finalize = c->merge_fin ? 1u : 0u;
    return F2V_OK;
}

int f2v_train(f2v_handle c, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode,
              double *seconds_out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (option == 1) {  // exact all-pairs: plain launches, nothing to snapshot or recover
        c->stats.snapshot_seconds = 0.0;
        c->stats.recovered = 0u;
        return train_exact(c, iters, batch, bs_mode, seconds_out);
    }
    // A launch whose workgroups wait for each other (combine-tree nodes inside the step kernel's grid, chained minibatches)
    // counts on this process having the GPU to itself: another process that fills the card with ITS waiting workgroups can
    // keep the ones everybody waits for from starting.  Every wait is bounded, and a wait that gives up must not cost the
    // caller its embeddings: the matrix and the rand() state are kept as they were when the call began ("recover", one more
    // matrix of HBM), and a call that loses a launch runs again from there with one launch per minibatch and per tree level
    // -- no in-grid waits, the same bits.
    bool snap = false;
    Rand rng0 = c->rng;
    const uint64_t fast_epoch0 = c->fast_epoch;
    if (c->waits_suspended && !c->merge_fin && ++c->calls_since_give_up > c->waits_backoff) {
        c->merge_fin = true;  // a recovered give-up is taken for a transient: the fast launch forms come back (with the net below)
        c->waits_suspended = false;
    }
    double snap_seconds = 0.0;
    if (c->recover && c->merge_fin && c->have_x && iters > 0) {  // (merge_fin: this handle's launches may hold in-grid waits)
        HIPC(hipSetDevice(c->device));
        int rc = flush_pending(c);
        if (rc != F2V_OK) return rc;
        const size_t bytes = (size_t)c->n * c->D * sizeof(float);
        if (c->d_snap.try_reserve((size_t)c->n * c->D)) {  // (no room for it: the call runs without the net)
            F2VC(c->snap_timer.start(c->stream));
            HIPC(hipMemcpyAsync(c->d_snap, c->d_X[c->cur], bytes, hipMemcpyDeviceToDevice, c->stream));
            F2VC(c->snap_timer.stop(c->stream));
            snap = true;
        }
    }
    const bool waits_before = c->merge_fin;
    int rc = train_impl(c, option, iters, batch, ns, lr, bs_mode, seconds_out, false);
    if (snap && hipEventQuery(c->snap_timer.ev[1]) == hipSuccess) {  // (train_impl has synchronised the stream on every healthy way out)
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->snap_timer.ev[0], c->snap_timer.ev[1]) == hipSuccess) snap_seconds = ms * 1e-3;
    }
    (void)hipGetLastError();
    bool recovered = false;
    if (rc == F2V_ESTATE && snap && c->x_invalid && !c->merge_fin) {
        const std::string why = f2v_last_error();
        HIPC(hipStreamSynchronize(c->stream));
        HIPC(hipMemcpyAsync(c->d_X[c->cur], c->d_snap, (size_t)c->n * c->D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        c->rng = rng0;
        c->fast_epoch = fast_epoch0;
        c->have_x = true;
        c->x_invalid = false;
        c->recoveries++;
        rc = train_impl(c, option, iters, batch, ns, lr, bs_mode, seconds_out, false);
        if (rc == F2V_OK) {
            recovered = true;
            (void)fail(F2V_OK, "f2v_train recovered: the call was run again from its start with one launch per minibatch and tree level after: %s", why.c_str());
            if (waits_before) {  // in-grid waits come back after a few healthy calls (doubling: 1, 2, 4 ... 64)
                c->waits_suspended = true;
                c->calls_since_give_up = 0;
                c->waits_backoff = c->recoveries <= 1 ? 1u : std::min(c->waits_backoff * 2u, 64u);
            }
        }
    }
    c->stats.snapshot_seconds = snap_seconds;
    c->stats.recovered = recovered ? 1u : 0u;
    return rc;
}

int f2v_train_marks(f2v_handle c, double *seconds_out, uint32_t cap, uint32_t *count_out) {
    if (!c || (cap && !seconds_out)) return fail(F2V_EINVAL, "f2v_train_marks: null argument");
    if (count_out) *count_out = (uint32_t)c->marks.size();
    for (uint32_t k = 0; k < cap && k < c->marks.size(); k++) seconds_out[k] = c->marks[k];
    return F2V_OK;
}

int f2v_objective(f2v_handle c, int option, uint32_t ns, f2v_objective_t *out) {
    if (!c || !out) return fail(F2V_EINVAL, "f2v_objective: null argument");
    const bool exact = option == 1;  // the all-pairs objective: ns is ignored
    if (!exact && !math_of_option(option)) return fail(F2V_EINVAL, "f2v_objective: option %d is neither 1 nor one of 5..11", option);
    if (c->n < 2) return fail(F2V_EINVAL, "f2v_objective: the graph needs at least two vertices");
    int rc = settled_enter(c, "f2v_objective");
    if (rc != F2V_OK) return rc;
    if ((rc = exact ? exact_objective_prepare(c) : objective_prepare(c)) != F2V_OK) return rc;
    rc = exact ? launch_exact_objective(c, c->d_X[c->cur], c->d_obj_out + kLossLogMax) : launch_objective(c, c->d_X[c->cur], option, ns, c->d_obj_out + kLossLogMax);
    if (rc != F2V_OK) return rc;
    ObjPartial r;
    HIPC(hipMemcpyAsync(&r, c->d_obj_out + kLossLogMax, sizeof r, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if ((rc = check_kernel_err(c, "f2v_objective")) != F2V_OK) return rc;
    out->attraction = r.attraction;
    out->repulsion = r.repulsion;
    out->loss = r.attraction + r.repulsion;
    out->positive_pairs = r.positive_pairs;
    out->negative_pairs = r.negative_pairs;
    return F2V_OK;
}

int f2v_train_losses(f2v_handle c, uint32_t *epochs_out, double *values_out, uint32_t cap, uint32_t *count_out) {
    if (!c || (cap && (!epochs_out || !values_out))) return fail(F2V_EINVAL, "f2v_train_losses: null argument");
    if (count_out) *count_out = (uint32_t)c->loss_epochs.size();
    for (uint32_t k = 0; k < cap && k < c->loss_epochs.size(); k++) {
        epochs_out[k] = c->loss_epochs[k];
        for (int v = 0; v < 3; v++) values_out[3 * k + v] = c->loss_values[3 * k + v];
    }
    return F2V_OK;
}

int f2v_train_sharded(f2v_handle c, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode,
                      double *seconds_out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (option == 1) return fail(F2V_EINVAL, "f2v_train_sharded: option 1 (exact all-pairs Force2Vec) runs on a single GPU, f2v_train only");
    if (c->loss_every) return fail(F2V_EINVAL, "f2v_train_sharded: \"loss_every\" is not supported (a rank does not hold the whole matrix between minibatches)");
    if (!c->push.attached) return fail(F2V_ESTATE, "f2v_train_sharded: f2v_push_attach first");
    const int math = math_of_option(option);
    c->last_replicated = false;
    if (math && batch && iters && !(math == 7 && bs_mode) && c->have_x && c->push.all_chain &&
        (c->replicate_small == 2 || (c->replicate_small == 1 && !c->push.any_shared))) {
        // Every rank must decide alike: the graph, the batch, the engine parameters (the callers set them alike on every rank, as they
        // must for the sharded form) and what f2v_push_attach learnt about ALL ranks.  Not this rank's "merge_finalize": a rank whose
        // in-grid waits are suspended after a recovered give-up still runs the whole epoch itself, one launch per minibatch -- same bits.
        const bool waits = c->merge_fin;
        c->merge_fin = true;
        const bool replicate = chain_usable(c, math, batch, bs_mode, false);
        c->merge_fin = waits;
        if (replicate) {
            c->push.rows_pushed = c->push.rows_allgather = 0;
            c->last_replicated = true;
            return f2v_train(c, option, iters, batch, ns, lr, bs_mode, seconds_out);
        }
    }
    return train_impl(c, option, iters, batch, ns, lr, bs_mode, seconds_out, true);
}

}  // extern "C"

namespace {

// f2v_train, and f2v_train_sharded when `sharded`: this rank computes its slice of every minibatch, pushes the new
// rows to the peers that read them and passes the flag barrier before the next minibatch.
int train_impl(f2v_ctx *c, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode, double *seconds_out, bool sharded) {
    const int math = math_of_option(option);
    if (!math) return fail(F2V_EINVAL, "f2v_train: option %d is outside 5..11", option);
    c->unit_degi = option == 10;
    if (!c->have_x) return fail(F2V_ESTATE, "f2v_train: embeddings not initialised (f2v_init_embeddings)");
    if (batch == 0) return fail(F2V_EINVAL, "f2v_train: batch must be positive");
    if (math == 7 && bs_mode) return fail(F2V_EINVAL, "option 7 has no -bs 1 variant");
    c->loss_epochs.clear();  // (a call run again from its snapshot starts the log afresh)
    c->loss_values.clear();
    c->last_loss_us = 0.0;
    if (c->loss_every && c->n < 2) return fail(F2V_EINVAL, "f2v_train: \"loss_every\" needs a graph of at least two vertices");
    HIPC(hipSetDevice(c->device));
    int rc;
    const uint32_t n = c->n;
    const uint32_t nb = (uint32_t)(((uint64_t)n + batch - 1) / batch);
    // rand() draws per minibatch: ns, or ns*BATCHSIZE with -bs 1 (algorithms.cpp:686, 966) of which rows+ns-1 are used
    const uint64_t ndraw = bs_mode ? (uint64_t)ns * batch : ns;
    const uint64_t stride = bs_mode ? (uint64_t)std::min(batch, n) + ns : ns;  // ids kept per minibatch
    const uint64_t per_epoch = (uint64_t)nb * stride;
    if (c->chunk_auto) {
        // sharded: a rank's launch covers batch/world rows, and its longest serial stretch (one chunk) has to
        // shrink with it or the step kernel stops getting shorter (measured on RMAT-20, B = 65536, 8 ranks: 87 us
        // per minibatch with the whole batch's chunk, 32 us with the slice's).  The chunk is part of the summation
        // order: results are bit-identical for any world size GIVEN the chunk ("hub_chunk" pins it).
        const uint32_t ch = auto_chunk(c, sharded ? (batch + c->push.world - 1) / c->push.world : batch);
        if (ch != c->chunk) {
            if ((rc = quiesce(c)) != F2V_OK) return rc;
            c->chunk = ch;
            drop_plans(c);
        }
    }
    // Sample ids do not depend on the embeddings: options 5/6 pre-draw every epoch's ids (as long
    // as that stays below 1 GiB); option 7 interleaves walk generation, so it goes epoch by epoch.
    const bool all_upfront = (math != 7 || c->fast_rng) && (per_epoch * iters * 4ull <= (1ull << 30));
    // small minibatches: groups of them in one launch (chain_plan_for), ordered by data dependencies instead of launch boundaries
    const bool chained = iters > 0 && chain_usable(c, math, batch, bs_mode, sharded);
    const bool wide = chained && wide_usable(c) && batch <= c->wide_max_batch && (chain_len(c, batch, true) >= 2 || c->wide_single);
    const uint32_t K = chained ? chain_len(c, batch, wide) : 1;
    uint32_t epochs_max = 1;  // "wide_epochs"
    if (wide && all_upfront && math != 7 && !bs_mode && ns <= 8 && !c->mark_every && !hooks_forbid_ring(c)) {
        epochs_max = c->wide_epochs ? c->wide_epochs : (c->nnz <= (2ull << 20) ? 32u : 1u);
        epochs_max = (uint32_t)std::min<uint64_t>(epochs_max, (8ull << 30) / std::max<uint64_t>((uint64_t)n * c->D * sizeof(float), 1));  // the ring stays below 8 GiB
        if (2ull * n * c->D * sizeof(float) > 0xFFFFFFFFull) epochs_max = 1;  // an epoch's two matrices of the ring are read at 32-bit byte offsets (load16_agent)
    }
    c->last_wide_epochs = 1;
    c->last_train_form = 0;  // (set where a launch is made: launch_step 0 / 3 under hipGraph replay, launch_chain 1, launch_wide 2)
    if (wide) {
        wide_plans_for_epoch(c, nb, K, batch, math == 7);
    } else if (chained) {
        for (uint32_t b0 = 0; b0 < nb; b0 += K) (void)chain_plan_for(c, b0, std::min(K, nb - b0), batch, math == 7);
    } else {
        for (uint32_t b = 0; b < nb; b++) {  // all launch plans up-front: one upload, no syncs inside the timed loop
            uint32_t lo = b * batch, hi = (uint32_t)std::min<uint64_t>((uint64_t)b * batch + batch, n);
            if (sharded) shard_of(c, math == 7, lo, hi, c->push.rank, c->push.world, &lo, &hi);
            (void)plan_for(c, lo, hi, math == 7);
        }
    }
    if ((rc = upload_plans(c)) != F2V_OK) return rc;
    // (epochs whose ids cannot all be drawn up-front alternate between two device buffers: reserved HERE, once -- a second, larger
    // reservation further down would hipFree the first, and hipFree waits for every stream of the device: with the ranks of a push
    // exchange as engines of ONE process (tools/push_world_local.py) that is a peer's spinning barrier kernel, which waits for this rank)
    const uint64_t dev_ids = std::max<uint64_t>(all_upfront ? per_epoch * std::max(iters, 1u) : 2 * per_epoch, 64);
    if ((rc = c->d_ids.reserve(c, dev_ids, "sample ids")) != F2V_OK) return rc;
    c->ids_valid = 0;
    std::vector<uint32_t> ids;
    auto draw_epoch = [&](std::vector<uint32_t> &v, size_t off) {
        for (uint32_t b = 0; b < nb; b++) {
            uint32_t maxv = n - 1;
            if (math == 7) {  // algorithms.cpp:1125 (option 10: :2124)
                const uint64_t e = (uint64_t)(b + 1) * batch;
                if (e < maxv) maxv = (uint32_t)e;
            }
            // option 9's own rule (AlgoForce2VecNSRW_SREAL_D128_AVXZ): full minibatches draw from [0, (b+1)*BATCHSIZE)
            // (algorithms.cpp:1700-1704; reaches vertex N-1 when the batch size divides N), the tail from [0, N-1) (:1939-1941)
            if (option == 9 && b < n / batch) maxv = (b + 1) * batch;
            for (uint64_t s = 0; s < ndraw; s++) {
                const uint32_t r = c->rng.index(maxv, 0);
                if (s < stride) v[off + (size_t)b * stride + s] = r;
            }
        }
    };
    if (chained && !c->d_rowflag) {
        F2VC(c->d_rowflag.reserve(c->n, "row flags"));
        HIPC(hipMemsetAsync(c->d_rowflag, 0, (size_t)c->n * sizeof(uint32_t), c->stream));  // 0 is no launch's sequence number
        HIPC(hipStreamSynchronize(c->stream));
    }
    if (all_upfront) {
        ids.assign(per_epoch * iters, 0u);
        for (uint32_t it = 0; it < iters; it++) draw_epoch(ids, (size_t)it * per_epoch);
        if (!ids.empty()) HIPC(hipMemcpy(c->d_ids, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    } else {
        ids.assign(per_epoch, 0u);
    }
    c->stats = f2v_stats{};
    // sharded: who reads which row is static when the neighbours are the CSR's and the run's sample ids are known
    // up-front; otherwise (option 7's walks, -bs 1's per-row sample windows) every new row goes to every peer
    const bool exchanging = sharded && c->push.world > 1;
    if (exchanging && c->push.landing && std::min(batch, n) > c->push.landing_cap)
        return fail(F2V_EINVAL, "f2v_train_sharded: a minibatch of %u rows does not fit the landing buffer (%u rows; matrices of 2 GiB and more are exchanged through it)", std::min(batch, n), c->push.landing_cap);
    const bool need_based = exchanging && math != 7 && !bs_mode && all_upfront;
    const uint32_t *d_masks = nullptr;
    if (need_based) {
        if ((rc = prepare_masks(c, batch, ids)) != F2V_OK) return rc;
        d_masks = c->push.d_masks;
    }
    if (sharded) c->push.rows_pushed = c->push.rows_allgather = 0;
    DevEvents events;  // destroyed on every way out of this function
    hipEvent_t ev0, ev1;
    std::vector<hipEvent_t> mark_ev;  // "epoch_marks"
    c->marks.clear();
    if ((rc = events.make(&ev0, hipEventDefault)) != F2V_OK || (rc = events.make(&ev1, hipEventDefault)) != F2V_OK) return rc;
    // "loss_every" = k: the objective of the matrix after epochs k, 2k, ... and after the last one, enqueued between the epochs (no
    // synchronisation, no allocation in the loop), each bracketed by a pair of events: their time is taken out of the epoch loop's and
    // the marks'.  The results stay on the device until the end of the call.
    const uint32_t loss_k = c->loss_every;
    const uint32_t loss_planned = loss_k ? std::min<uint32_t>(iters / loss_k + (iters % loss_k ? 1u : 0u), kLossLogMax) : 0u;
    std::vector<hipEvent_t> loss_ev(2 * (size_t)loss_planned);
    std::vector<uint32_t> loss_log;  // the epochs of the evaluations enqueued so far
    std::vector<size_t> mark_loss;   // evaluations enqueued before each mark
    if (loss_planned) {
        if ((rc = objective_prepare(c)) != F2V_OK) return rc;
        for (auto &e : loss_ev)
            if ((rc = events.make(&e, hipEventDefault)) != F2V_OK) return rc;
    }
    auto loss_due = [&](uint32_t g) { return loss_k && (g % loss_k == 0 || g == iters) && loss_log.size() < loss_planned; };
    auto evaluate = [&](uint32_t g, const float *X) -> int {  // epoch g (1-based) left matrix X
        const size_t m = loss_log.size();
        HIPC(hipEventRecord(loss_ev[2 * m], c->stream));
        const int r = launch_objective(c, X, option, ns, c->d_obj_out + m);
        if (r != F2V_OK) return r;
        HIPC(hipEventRecord(loss_ev[2 * m + 1], c->stream));
        loss_log.push_back(g);
        return F2V_OK;
    };
    HIPC(hipEventRecord(ev0, c->stream));
#ifdef F2V_TEST_HOOKS
    // F2V_PUSH_CHAOS=<seed> (self-test build only): every rank stalls at random minibatches (different ones on every rank)
    unsigned long long chaos = 0;
    if (const char *e = getenv("F2V_PUSH_CHAOS")) chaos = (strtoull(e, nullptr, 10) + 1) * 0x9E3779B97F4A7C15ull + c->push.rank * 0xD1B54A32D192ED03ull;
#endif
    // The kernels' error words (a combine-tree wait that gave up) are copied to pinned memory at the end of every epoch,
    // stream-ordered, and looked at without blocking as soon as the copy has run: a lost run fails within an epoch or two
    // of the give-up instead of at its very end.  Four copies may be in flight (ring of events / 64-byte slots of h_kerr).
    constexpr int kErrRing = 4;
    uint32_t err_seq = 0;
    hipEvent_t err_ev[kErrRing];
    bool err_used[kErrRing] = {};
    for (auto &e : err_ev)
        if ((rc = events.make(&e, hipEventDisableTiming)) != F2V_OK) return rc;
    auto poll_errors = [&](bool wait_slot, int slot) -> const uint32_t * {  // -> the error words if some epoch gave up
        for (int k = 0; k < kErrRing; k++) {
            if (!err_used[k]) continue;
            if (wait_slot && k == slot) (void)hipEventSynchronize(err_ev[k]);
            else if (hipEventQuery(err_ev[k]) != hipSuccess) continue;
            err_used[k] = false;
            if (c->h_kerr[16 * k]) return c->h_kerr + 16 * k;
        }
        return nullptr;
    };
    const bool graphed = c->use_graph && math != 7 && all_upfront && iters >= 2 && !sharded;
    if (graphed) {
        c->last_train_form = 3;  // one launch per minibatch and tree level, replayed from two captured graphs
        // hipGraph replay: an epoch's launch chain is identical every epoch except for (a) which of the two matrices
        // is read and which written -- they alternate, hence one graph per epoch parity -- and (b) the sample ids,
        // which each replay finds at a fixed place (its parity's region of d_ids), refreshed by a stream-ordered copy.
        hipGraph_t graph[2] = {nullptr, nullptr};
        hipGraphExec_t exec[2] = {nullptr, nullptr};
        if (loss_planned && (rc = flush_pending(c)) != F2V_OK) return rc;  // (what the first captured step would do): epoch e then reads
        const int cur0 = c->cur;                                             // d_X[cur0 ^ (e & 1)] and writes the other one
        for (int par = 0; par < 2; par++) {
            HIPC(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            c->capturing = true;  // a replayed launch cannot carry a fresh sequence number: one launch per tree level
            for (uint32_t b = 0; b < nb && rc == F2V_OK; b++) {
                const uint32_t lo = b * batch;
                const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + batch, n);
                rc = launch_step(c, math, lo, hi, lo, hi, c->d_ids + (size_t)par * per_epoch + (size_t)b * stride, ns, lr, bs_mode);
            }
            hipError_t e = hipStreamEndCapture(c->stream, &graph[par]);
            c->capturing = false;
            if (rc != F2V_OK) return rc;
            HIPC(e);
            HIPC(hipGraphInstantiate(&exec[par], graph[par], nullptr, nullptr, 0));
        }
        // the host-side bookkeeping now stands where two executed epochs leave it; one epoch's statistics were counted twice
        f2v_stats one = c->stats;
        scale_stats(one, 1, 2);
        HIPC(hipEventRecord(ev0, c->stream));
        for (uint32_t it = 0; it < iters; it++) {
            if (it >= 2)
                HIPC(hipMemcpyAsync(c->d_ids + (size_t)(it & 1) * per_epoch, ids.data() + (size_t)it * per_epoch, per_epoch * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, c->stream));
            HIPC(hipGraphLaunch(exec[it & 1], c->stream));
            if (loss_due(it + 1) && (rc = evaluate(it + 1, c->d_X[cur0 ^ ((it + 1) & 1)])) != F2V_OK) return rc;
        }
        if (iters & 1) c->cur ^= 1;  // an odd number of epochs ends on the other matrix than the two captured ones did
        c->stats = one;
        scale_stats(c->stats, iters, 1);
        HIPC(hipStreamSynchronize(c->stream));
        for (int par = 0; par < 2; par++) { (void)hipGraphExecDestroy(exec[par]); (void)hipGraphDestroy(graph[par]); }
    }
    // Epochs whose host-side inputs cannot all be drawn up-front (option 7: the walks are 5 N ids per epoch, and the one serial
    // rand() stream interleaves them with the sample ids): a producer thread draws epoch e+1's walks and ids -- they never depend
    // on the embeddings (sample/algorithms.cpp:1097-1132) -- into pinned buffers while the device runs epoch e; the copies are
    // stream-ordered asynchronous copies into alternating device buffers, and nothing in the loop waits for the device.
    // Epoch time = max(host generation, device), instead of their sum plus two synchronisations.
    struct HostEpoch {
        HostBuf<uint32_t> walks, ids;
        hipEvent_t copied = nullptr;  // the H2D copies out of this slot have completed (one of `events`)
        bool full = false, copy_pending = false;
    } slot[2];  // (declared before producer_guard: freed behind it, once the thread has ended and no copy reads them)
    std::mutex mu;
    std::condition_variable cv;
    std::thread producer;
    bool stop_producer = false;
    const bool host_walks = (math == 7 && !c->fast_rng);
    const bool produced = !all_upfront && !graphed && iters > 0;
    uint32_t *walks_at[2] = {nullptr, nullptr};  // the device's walk buffers: epoch `it` of this call uses walks_at[it & 1]
    auto end_producer = [&] {
        if (producer.joinable()) {
            { std::lock_guard<std::mutex> lk(mu); stop_producer = true; }
            cv.notify_all();
            producer.join();
        }
        if (slot[0].copy_pending || slot[1].copy_pending) (void)hipStreamSynchronize(c->stream);  // no copy still reads the pinned buffers
    };
    struct AtExit {
        std::function<void()> f;
        ~AtExit() { f(); }
    } producer_guard{end_producer};  // every return below joins the thread and waits for the copies out of the pinned buffers
    if (produced) {
        const size_t nwalk = (size_t)n * kWalkLength;
        if (host_walks) {
            for (auto &b : c->d_walk_buf) F2VC(b.reserve(nwalk, "walks"));
            const int first = c->d_walks == c->d_walk_buf[1] ? 1 : 0;  // the current buffer takes the first epoch's walks
            walks_at[0] = c->d_walk_buf[first];
            walks_at[1] = c->d_walk_buf[first ^ 1];
        }
        if ((rc = c->d_ids.reserve(c, std::max<uint64_t>(2 * per_epoch, 64), "sample ids")) != F2V_OK) return rc;
        for (auto &sl : slot) {
            if (host_walks) F2VC(sl.walks.reserve(nwalk));
            F2VC(sl.ids.reserve(per_epoch));
            F2VC(events.make(&sl.copied, hipEventDisableTiming));
        }
        const int dev = c->device;
        producer = std::thread([&, dev] {
            (void)hipSetDevice(dev);
            std::vector<uint32_t> w, v(per_epoch);
            for (uint32_t it = 0; it < iters; it++) {
                HostEpoch &sl = slot[it & 1];
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop_producer || !sl.full; });
                    if (stop_producer) return;
                }
                if (sl.copy_pending) { (void)hipEventSynchronize(sl.copied); sl.copy_pending = false; }  // the slot's last copies have left it
                if (host_walks) {  // the reference's order: the epoch's walks, then its minibatches' sample ids
                    generate_walks_host(c, w);
                    memcpy(sl.walks, w.data(), w.size() * sizeof(uint32_t));
                }
                draw_epoch(v, 0);
                if (per_epoch) memcpy(sl.ids, v.data(), per_epoch * sizeof(uint32_t));
                { std::lock_guard<std::mutex> lk(mu); sl.full = true; }
                cv.notify_all();
            }
        });
    }
    for (uint32_t it = 0; it < iters && !graphed; it++) {
        if (math == 7 && c->fast_rng) {
            if ((rc = fast_walks(c)) != F2V_OK) return rc;  // stream-ordered: no host work, no synchronisation
        }
        const uint32_t *d_epoch_ids = c->d_ids + (all_upfront ? (size_t)it * per_epoch : (size_t)(it & 1) * per_epoch);
        if (produced) {
            HostEpoch &sl = slot[it & 1];
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return sl.full; });
            }
            // stream-ordered behind epoch it-2's kernels, the last readers of these device buffers
            hipError_t he = hipSuccess;
            if (host_walks) {
                he = hipMemcpyAsync(walks_at[it & 1], sl.walks, (size_t)n * kWalkLength * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
                c->d_walks = walks_at[it & 1];
                c->have_walks = true;
            }
            if (he == hipSuccess && per_epoch)
                he = hipMemcpyAsync(c->d_ids + (size_t)(it & 1) * per_epoch, sl.ids, per_epoch * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            if (he == hipSuccess) he = hipEventRecord(sl.copied, c->stream);
            {
                std::lock_guard<std::mutex> lk(mu);
                sl.copy_pending = true;
                sl.full = false;
            }
            cv.notify_all();
            HIPC(he);
        }
        if (wide) {
            for (uint32_t b0 = 0; b0 < nb; b0 += K) {
                const WidePlan plan = wide_plan_for(c, b0, std::min(K, nb - b0), batch, math == 7);
                if ((rc = upload_plans(c)) != F2V_OK) return rc;
                // epochs chained in one launch: the plan covers the graph, every epoch's sample ids are on the device, no walks, no marks
                uint32_t E = 1;
                if (epochs_max > 1 && K >= nb && plan.n_node_wgs == 0 && !c->ring_refused) E = std::min(epochs_max, iters - it);
                if ((rc = launch_wide(c, math, plan, d_epoch_ids, (uint32_t)stride, ns, lr, bs_mode, &E, per_epoch)) != F2V_OK) return rc;
                for (uint32_t e = 0; e + 1 < E; e++) {  // epochs inside a multi-epoch launch: epoch e left matrix e + 1 of its ring
                    if (loss_due(it + e + 1) && (rc = evaluate(it + e + 1, c->d_ring + (size_t)(e + 1) * n * c->D)) != F2V_OK) return rc;
                }
                it += E - 1;
            }
        } else if (chained) {
            for (uint32_t b0 = 0; b0 < nb; b0 += K) {
                const ChainPlan plan = chain_plan_for(c, b0, std::min(K, nb - b0), batch, math == 7);
                if ((rc = upload_plans(c)) != F2V_OK) return rc;  // O(1) unless the plan cache was dropped meanwhile
                if ((rc = launch_chain(c, math, plan, d_epoch_ids, (uint32_t)stride, ns, lr, bs_mode)) != F2V_OK) return rc;
            }
        }
        for (uint32_t b = 0; b < nb && !chained; b++) {
            const uint32_t lo = b * batch;
            const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + batch, n);
            uint32_t my_lo = lo, my_hi = hi;
            if (sharded) shard_of(c, math == 7, lo, hi, c->push.rank, c->push.world, &my_lo, &my_hi);
#ifdef F2V_TEST_HOOKS
            if (exchanging && chaos) {  // random host-side stalls skew the ranks against each other
                chaos = chaos * 6364136223846793005ull + 1442695040888963407ull;
                if (((chaos >> 33) & 7u) == 0u) {
                    HIPC(hipStreamSynchronize(c->stream));
                    std::this_thread::sleep_for(std::chrono::microseconds((chaos >> 40) % 3000u));
                }
            }
#endif
            if ((rc = launch_step(c, math, lo, hi, my_lo, my_hi, d_epoch_ids + (size_t)b * stride, ns, lr, bs_mode, exchanging && c->push.fused, d_masks)) != F2V_OK) return rc;
            if (exchanging) {
                if (!c->push.fused && (rc = launch_push(c, c->cur ^ 1, d_masks, lo, my_lo, my_hi)) != F2V_OK) return rc;
                if ((rc = finish_exchange(c, c->cur ^ 1, d_masks, lo, hi, my_lo, my_hi)) != F2V_OK) return rc;
                c->push.rows_allgather += (uint64_t)(my_hi - my_lo) * (c->push.world - 1);
            }
        }
        if (exchanging) c->push.rows_pushed += need_based ? c->push.pushed_per_epoch : (uint64_t)0;
        if (c->mark_every && (it + 1) % c->mark_every == 0 && mark_ev.size() < 4096) {
            hipEvent_t e;
            if ((rc = events.make(&e, hipEventDefault)) != F2V_OK) return rc;
            HIPC(hipEventRecord(e, c->stream));
            mark_ev.push_back(e);
            mark_loss.push_back(loss_log.size());
        }
        if (loss_due(it + 1)) {
            const float *X = settled_matrix(c);
            if (!X) {
                if ((rc = flush_pending(c)) != F2V_OK) return rc;
                X = c->d_X[c->cur];
            }
            if ((rc = evaluate(it + 1, X)) != F2V_OK) return rc;
        }
        if (c->merge_fin) {
            const int slot = (int)(err_seq++ % kErrRing);  // (by copies made, not by epoch: a launch may carry 32 epochs)
            const uint32_t *bad = poll_errors(err_used[slot], slot);  // the slot about to be reused is waited for (4 epochs old)
            if (!bad) {
                HIPC(hipMemcpyAsync(c->h_kerr + 16 * slot, c->d_kerr, 64, hipMemcpyDeviceToHost, c->stream));
                HIPC(hipEventRecord(err_ev[slot], c->stream));
                err_used[slot] = true;
            } else {
                uint32_t e[16];
                memcpy(e, bad, sizeof e);
                char where[96];
                snprintf(where, sizeof where, "%s (noticed after epoch %u of %u)", sharded ? "f2v_train_sharded" : "f2v_train", it + 1, iters);
                return kernel_gave_up(c, where, e);
            }
        }
    }
    if (exchanging && !need_based) c->push.rows_pushed = c->push.rows_allgather;
    if ((rc = flush_pending(c)) != F2V_OK) return rc;
    if (need_based && iters > 0) {
        // replicas are complete only in the rows their rank reads: one full exchange makes them whole
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t lo = b * batch, hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + batch, n);
            uint32_t my_lo, my_hi;
            shard_of(c, math == 7, lo, hi, c->push.rank, c->push.world, &my_lo, &my_hi);
            if ((rc = launch_push(c, c->cur, nullptr, lo, my_lo, my_hi)) != F2V_OK) return rc;
            // the landing buffer holds one minibatch: an exchange per minibatch; mapped matrices take them all at once
            if (c->push.landing && (rc = finish_exchange(c, c->cur, nullptr, lo, hi, my_lo, my_hi)) != F2V_OK) return rc;
        }
        if (!c->push.landing && (rc = launch_barrier(c)) != F2V_OK) return rc;
    }
    HIPC(hipEventRecord(ev1, c->stream));
    HIPC(hipEventSynchronize(ev1));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ev0, ev1));
    std::vector<double> loss_ms(loss_log.size() + 1, 0.0);  // evaluation time before entry m: not the epoch loop's
    for (size_t m = 0; m < loss_log.size(); m++) {
        float em = 0.f;
        HIPC(hipEventElapsedTime(&em, loss_ev[2 * m], loss_ev[2 * m + 1]));
        loss_ms[m + 1] = loss_ms[m] + em;
    }
    c->last_loss_us = loss_ms.back() * 1e3;
    c->stats.device_seconds = loss_log.empty() ? ms * 1e-3 : (ms - loss_ms.back()) * 1e-3;
    if (seconds_out) *seconds_out = c->stats.device_seconds;
    for (size_t k = 0; k < mark_ev.size(); k++) {
        float mm = 0.f;
        HIPC(hipEventElapsedTime(&mm, ev0, mark_ev[k]));
        c->marks.push_back(loss_log.empty() ? mm * 1e-3 : (mm - loss_ms[mark_loss[k]]) * 1e-3);
    }
    if ((rc = check_kernel_err(c, sharded ? "f2v_train_sharded" : "f2v_train")) != F2V_OK) return rc;
    if (!loss_log.empty()) {  // the log's one copy to the host
        std::vector<ObjPartial> r(loss_log.size());
        HIPC(hipMemcpy(r.data(), c->d_obj_out, r.size() * sizeof(ObjPartial), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < r.size(); m++) {
            c->loss_epochs.push_back(loss_log[m]);
            c->loss_values.insert(c->loss_values.end(), {r[m].attraction + r[m].repulsion, r[m].attraction, r[m].repulsion});
        }
    }
    if (exchanging) return check_push_err(c, "f2v_train_sharded");
    return F2V_OK;
}

// ---- exact all-pairs Force2Vec, option 1 (f2v_exact.hip.h; definition in include/f2v.h) -----------------------------------------
uint32_t exact_spans(const f2v_ctx *c) { return (c->n + kExactSpanCols - 1u) / kExactSpanCols; }

// STEP_e: e multiplications from 1.0f (sample/algorithms.cpp:436, the product formed in fp64 as the reference's 0.999 is a double)
float exact_step(uint64_t e) {
    float step = 1.0f;
    for (uint64_t k = 0; k < e; k++) step = (float)((double)step * 0.999);
    return step;
}

template <int VEC, bool EXACT>
void launch_exact_pair_t(f2v_ctx *c, const ExactArgs &a, uint32_t rows_per_wg) {
    const uint32_t groups = (a.hi - a.lo + rows_per_wg - 1u) / rows_per_wg;
    const dim3 grid(groups, a.spans + 1u);
    if (rows_per_wg == 4) hipLaunchKernelGGL((exact_pair_kernel<VEC, EXACT, 1>), grid, dim3(256), 0, c->stream, a);
    else if (rows_per_wg == 8) hipLaunchKernelGGL((exact_pair_kernel<VEC, EXACT, 2>), grid, dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL((exact_pair_kernel<VEC, EXACT, 4>), grid, dim3(256), 0, c->stream, a);
}

// the same launch in the quarter-wave layout (D a multiple of 4 up to 256, "quarter_wave" on): one wavefront per four rows
void launch_exact_pair_q(f2v_ctx *c, const ExactArgs &a, uint32_t rows_per_wg) {
    const dim3 grid((a.hi - a.lo + rows_per_wg - 1u) / rows_per_wg, a.spans + 1u), block(16u * rows_per_wg);
    if (c->D <= 64u) hipLaunchKernelGGL((exact_pair_q_kernel<1>), grid, block, 0, c->stream, a);
    else if (c->D <= 128u) hipLaunchKernelGGL((exact_pair_q_kernel<2>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((exact_pair_q_kernel<4>), grid, block, 0, c->stream, a);
}

// Rows per workgroup ("exact_rows"): more rows share a staged column, fewer rows make more workgroups.  0: the most rows that
// still leave four workgroups per compute unit (1024 of them), from the minibatch's rows and the spans alone.
uint32_t exact_rows_per_wg(const f2v_ctx *c, uint32_t rows) {
    if (c->ex.rows) return c->ex.rows;
    const uint64_t slices = (uint64_t)exact_spans(c) + 1u;
    for (uint32_t r = 16; r > 4; r >>= 1)
        if ((uint64_t)((rows + r - 1u) / r) * slices >= 1024u) return r;
    return 4;
}

// One evaluation of the exact objective of matrix X (two launches, no synchronisation, no allocation once the workspace stands)
int launch_exact_objective(f2v_ctx *c, const float *X, ObjPartial *out) {
    ExactObjArgs a{};
    a.X = X;
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.row_att = c->ex.d_rows;
    a.row_rep = c->ex.d_rows + c->n;
    a.n = c->n;
    a.D = c->D;
    const uint32_t wgs = (c->n + 15u) / 16u;
    int rc = dispatch_layout(c, [&](auto V, auto E) {
        hipLaunchKernelGGL((exact_objective_kernel<decltype(V)::value, decltype(E)::value>), dim3(wgs), dim3(256), 0, c->stream, a);
    });
    if (rc != F2V_OK) return rc;
    HIPC(hipGetLastError());
    hipLaunchKernelGGL(exact_objective_reduce_kernel, dim3(1), dim3(1024), 0, c->stream, (const double *)a.row_att, (const double *)a.row_rep, c->n,
                       (unsigned long long)c->nnz, (double *)c->ex.d_piece, out);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// the exact objective's workspace (2 n doubles of row sums, 2 ceil(n / 64) doubles of piece sums) and the slots of the results
int exact_objective_prepare(f2v_ctx *c) {
    F2VC(objective_prepare(c));
    F2VC(c->ex.d_rows.reserve(c, 2 * (size_t)c->n, "exact objective"));
    return c->ex.d_piece.reserve(c, 2 * (size_t)((c->n + kExactPiece - 1u) / kExactPiece), "exact objective");
}

// f2v_train with option 1: per minibatch one launch of the pair kernel and one of the finish kernel on the handle's stream.  No
// in-grid waits (hence no snapshot and nothing to recover from), no rand() draw.
int train_exact(f2v_ctx *c, uint32_t iters, uint32_t batch, int bs_mode, double *seconds_out) {
    if (!c->have_x) return fail(F2V_ESTATE, "f2v_train: embeddings not initialised (f2v_init_embeddings)");
    if (batch == 0) return fail(F2V_EINVAL, "f2v_train: batch must be positive");
    if (bs_mode) return fail(F2V_EINVAL, "f2v_train: option 1 has no -bs 1 variant");
    if (c->loss_every && c->n < 2) return fail(F2V_EINVAL, "f2v_train: \"loss_every\" needs a graph of at least two vertices");
    c->loss_epochs.clear();
    c->loss_values.clear();
    c->last_loss_us = 0.0;
    c->marks.clear();
    HIPC(hipSetDevice(c->device));
    F2VC(flush_pending(c));
    const uint32_t n = c->n, D = c->D;
    const uint32_t nb = (uint32_t)(((uint64_t)n + batch - 1) / batch);
    const uint32_t spans = exact_spans(c);
    F2VC(c->ex.d_ws.reserve(c, (size_t)std::min(batch, n) * (spans + 1u) * D, "exact training"));
    c->stats = f2v_stats{};
    c->last_train_form = 0;
    c->last_wide_epochs = 1;
    DevEvents events;  // destroyed on every way out of this function
    hipEvent_t ev0, ev1;
    F2VC(events.make(&ev0));
    F2VC(events.make(&ev1));
    // "loss_every" and "epoch_marks" as train_impl has them: evaluations between the epochs, bracketed by events, their time taken out
    const uint32_t loss_k = c->loss_every;
    const uint32_t loss_planned = loss_k ? std::min<uint32_t>(iters / loss_k + (iters % loss_k ? 1u : 0u), kLossLogMax) : 0u;
    std::vector<hipEvent_t> loss_ev(2 * (size_t)loss_planned), mark_ev;
    std::vector<uint32_t> loss_log;
    std::vector<size_t> mark_loss;
    if (loss_planned) {
        F2VC(exact_objective_prepare(c));
        for (auto &e : loss_ev) F2VC(events.make(&e));
    }
    ExactArgs a{};
    a.X = c->d_X[c->cur];
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.ws = c->ex.d_ws;
    a.n = n;
    a.D = D;
    a.spans = spans;
    float step = exact_step(c->ex.epoch);
    HIPC(hipEventRecord(ev0, c->stream));
    for (uint32_t it = 0; it < iters; it++) {
        a.step = step;
        for (uint32_t b = 0; b < nb; b++) {
            a.lo = b * batch;
            a.hi = (uint32_t)std::min<uint64_t>((uint64_t)a.lo + batch, n);
            const uint32_t rows = a.hi - a.lo, rpw = exact_rows_per_wg(c, rows);
            // Both pair kernels give the same bits.  The quarter-wave one is the faster where a minibatch fills the card (measured
            // 1.5 x at 16384 rows, 1.2 x at 2708), the generic one at the reference's default-sized minibatches (1.1-1.35 x at 256
            // and 384 rows: its workgroups are always four wavefronts that share a staged piece): profiles/exact_time.txt.
            const bool quarter = subwave_width(c) != 0u && rows >= c->ex.quarter_min;
            c->ex.last_rows = rpw;
            c->ex.last_quarter = quarter;
            if (quarter) {
                launch_exact_pair_q(c, a, rpw);
            } else {
                int rc = dispatch_layout(c, [&](auto V, auto E) { launch_exact_pair_t<decltype(V)::value, decltype(E)::value>(c, a, rpw); });
                if (rc != F2V_OK) return rc;
            }
            HIPC(hipGetLastError());
            hipLaunchKernelGGL(exact_finish_kernel, dim3((uint32_t)(((size_t)rows * D + 255u) / 256u)), dim3(256), 0, c->stream, a);
            HIPC(hipGetLastError());
            c->stats.step_launches++;
            c->stats.rows += rows;
            c->stats.nnz += c->rowptr[a.hi] - c->rowptr[a.lo];
            // the columns of all n vertices and the minibatch's rows in, the span sums out and in again, the rows out
            c->stats.algorithmic_bytes += ((uint64_t)n + 2ull * rows + 2ull * rows * (spans + 1u)) * D * sizeof(float);
        }
        step = (float)((double)step * 0.999);
        if (c->mark_every && (it + 1) % c->mark_every == 0 && mark_ev.size() < 4096) {
            hipEvent_t e;
            F2VC(events.make(&e));
            HIPC(hipEventRecord(e, c->stream));
            mark_ev.push_back(e);
            mark_loss.push_back(loss_log.size());
        }
        if (loss_k && ((it + 1) % loss_k == 0 || it + 1 == iters) && loss_log.size() < loss_planned) {
            const size_t m = loss_log.size();
            HIPC(hipEventRecord(loss_ev[2 * m], c->stream));
            F2VC(launch_exact_objective(c, a.X, c->d_obj_out + m));
            HIPC(hipEventRecord(loss_ev[2 * m + 1], c->stream));
            loss_log.push_back(it + 1);
        }
    }
    HIPC(hipEventRecord(ev1, c->stream));
    HIPC(hipEventSynchronize(ev1));
    c->ex.epoch += iters;
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ev0, ev1));
    std::vector<double> loss_ms(loss_log.size() + 1, 0.0);  // evaluation time before entry m: not the epoch loop's
    for (size_t m = 0; m < loss_log.size(); m++) {
        float em = 0.f;
        HIPC(hipEventElapsedTime(&em, loss_ev[2 * m], loss_ev[2 * m + 1]));
        loss_ms[m + 1] = loss_ms[m] + em;
    }
    c->last_loss_us = loss_ms.back() * 1e3;
    c->stats.device_seconds = (ms - loss_ms.back()) * 1e-3;
    if (seconds_out) *seconds_out = c->stats.device_seconds;
    for (size_t k = 0; k < mark_ev.size(); k++) {
        float mm = 0.f;
        HIPC(hipEventElapsedTime(&mm, ev0, mark_ev[k]));
        c->marks.push_back((mm - loss_ms[mark_loss[k]]) * 1e-3);
    }
    if (!loss_log.empty()) {
        std::vector<ObjPartial> r(loss_log.size());
        HIPC(hipMemcpy(r.data(), c->d_obj_out, r.size() * sizeof(ObjPartial), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < r.size(); m++) {
            c->loss_epochs.push_back(loss_log[m]);
            c->loss_values.insert(c->loss_values.end(), {r[m].attraction + r[m].repulsion, r[m].attraction, r[m].repulsion});
        }
    }
    return F2V_OK;
}

// ---- nearest-neighbour queries (f2v_nearest.hip.h; definition in include/f2v.h) -------------------------------------------------
template <bool L2, int WQ, int MI, int NI>
int launch_nearest_t(f2v_ctx *c, const NnArgs &a, uint32_t qblocks, uint32_t splits) {
    const size_t lds = nn_lds_bytes(32u * WQ * MI, a.D);
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&nearest_kernel<L2, WQ, MI, NI>), lds));
    hipLaunchKernelGGL((nearest_kernel<L2, WQ, MI, NI>), dim3(qblocks, splits), dim3(kNnThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// What the three entry points share behind their preamble.  Queries are rows `qids` of the matrix (nullptr with `all`: rows 0 .. nq-1)
// or the host vectors `vecs`; they are run in chunks of "nearest_chunk" queries, each chunk as gather / norms / nearest_kernel /
// merge (/ count) on the handle's stream between two events.  ids_out / scores_out may be nullptr (the recall count needs neither).
// `X`: the n x D matrix that is searched -- the handle's, or f2v_trustworthiness's second matrix (row queries, no cosine, no CSR flag);
// `d_ids_dst` (may be nullptr): device array that also receives the ids, nq x k; `d_scores_dst`: the same for the scores; `n_rows`
// (0: n): the rows of `X` where it is not a matrix over the vertices (f2v_tsne_affinities' gathered sample, the index's centroids);
// `vecs_on_device`: `vecs` is a device array (the index's staged queries).
int nearest_run_on(f2v_ctx *c, const float *X, uint32_t D, const uint32_t *qids, bool all, const float *vecs, uint32_t nq, uint32_t k, int metric,
                   uint32_t flags, uint32_t *ids_out, float *scores_out, uint64_t *recall_out, double *seconds_out, uint32_t *d_ids_dst,
                   float *d_scores_dst = nullptr, uint32_t n_rows = 0, bool vecs_on_device = false) {
    f2v_ctx::Nearest &w = c->nn;
    const uint32_t n = n_rows ? n_rows : c->n;
    const bool rows = qids || all, cosine = metric == F2V_SIM_COSINE;
    const char *what = "nearest-neighbour";
    F2VC(w.d_counts.reserve(c, 2, what));
    if (recall_out) HIPC(hipMemsetAsync(w.d_counts, 0, 2 * sizeof(unsigned long long), c->stream));
    if (cosine) F2VC(w.d_rc.reserve(c, n, what));
    const uint32_t tiles = (n + kNnTile - 1) / kNnTile;
    double seconds = 0.0;
    std::vector<uint32_t> iota;
    for (uint32_t done = 0; done < nq; done += w.chunk) {
        const uint32_t cq = std::min(w.chunk, nq - done);
        const uint32_t qb = w.block && !(w.block == 128 && D > 128) ? w.block : (D <= 128 && cq > 32 ? 128u : 32u);
        const uint32_t qblocks = (cq + qb - 1) / qb;
        uint32_t splits = w.splits;
        if (!splits)  // enough workgroups for every CU a few times over, but never more keys per query than the merge reads quickly
            splits = std::min({(1024u + qblocks - 1) / qblocks, std::max(1u, 8192u / k), 256u});
        splits = std::min(splits, tiles);
        const uint32_t tps = (tiles + splits - 1) / splits;
        splits = (tiles + tps - 1) / tps;
        const size_t keys = (size_t)qblocks * qb * splits * k, slots = (size_t)cq * k;
        F2VC(w.d_rq.reserve(c, cq, what));
        F2VC(w.d_qids.reserve(c, cq, what));
        F2VC(w.d_Q.reserve(c, (size_t)cq * D, what));
        F2VC(w.d_ws.reserve(c, keys, what));
        F2VC(w.d_ids.reserve(c, slots, what));
        F2VC(w.d_scores.reserve(c, slots, what));
        if (all) {
            iota.resize(cq);
            for (uint32_t i = 0; i < cq; i++) iota[i] = done + i;
        }
        if (rows) HIPC(hipMemcpyAsync(w.d_qids, all ? iota.data() : qids + done, (size_t)cq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        else HIPC(hipMemcpyAsync(w.d_Q, vecs + (size_t)done * D, (size_t)cq * D * sizeof(float), vecs_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        F2VC(w.timer.start(c->stream));
        if (rows) hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)cq * D + 255) / 256, 4096)), dim3(256), 0, c->stream, X, (const uint32_t *)w.d_qids, cq, D, w.d_Q);
        if (cosine) {
            if (done == 0) hipLaunchKernelGGL(nearest_rnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, X, n, D, w.d_rc);
            hipLaunchKernelGGL(nearest_rnorm_kernel, dim3((cq + 255) / 256), dim3(256), 0, c->stream, (const float *)w.d_Q, cq, D, w.d_rq);
        }
        HIPC(hipGetLastError());
        NnArgs a{};
        a.X = X;
        a.Q = w.d_Q;
        a.rq = cosine ? w.d_rq : nullptr;
        a.rc = cosine ? w.d_rc : nullptr;
        a.qids = rows ? w.d_qids : nullptr;
        a.rowptr = c->d_rowptr;
        a.colids = c->d_colids;
        a.ws = w.d_ws;
        a.n = n;
        a.D = D;
        a.nq = cq;
        a.k = k;
        a.flags = flags;
        a.splits = splits;
        a.tiles_per_split = tps;
        a.cosine = cosine ? 1u : 0u;
        if (metric == F2V_SIM_L2) F2VC((qb == 128 ? launch_nearest_t<true, 2, 2, 2>(c, a, qblocks, splits) : launch_nearest_t<true, 1, 1, 1>(c, a, qblocks, splits)));
        else F2VC((qb == 128 ? launch_nearest_t<false, 2, 2, 2>(c, a, qblocks, splits) : launch_nearest_t<false, 1, 1, 1>(c, a, qblocks, splits)));
        hipLaunchKernelGGL(nearest_merge_kernel, dim3(cq), dim3(256), 0, c->stream, (const nn_key_t *)w.d_ws, splits, k, w.d_ids, w.d_scores);
        if (recall_out)
            hipLaunchKernelGGL(nearest_recall_kernel, dim3((cq + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)w.d_ids, (const uint32_t *)w.d_qids, cq, k,
                               (const uint32_t *)c->d_rowptr, (const uint32_t *)c->d_colids, w.d_counts);
        HIPC(hipGetLastError());
        if (d_ids_dst) HIPC(hipMemcpyAsync(d_ids_dst + (size_t)done * k, w.d_ids, slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        if (d_scores_dst) HIPC(hipMemcpyAsync(d_scores_dst + (size_t)done * k, w.d_scores, slots * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        F2VC(w.timer.stop(c->stream));
        if (ids_out) HIPC(hipMemcpyAsync(ids_out + (size_t)done * k, w.d_ids, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (scores_out) HIPC(hipMemcpyAsync(scores_out + (size_t)done * k, w.d_scores, slots * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    F2VC(check_kernel_err(c, "nearest-neighbour query"));
    if (recall_out) {
        HIPC(hipMemcpyAsync(recall_out, w.d_counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

int nearest_run(f2v_ctx *c, const uint32_t *qids, bool all, const float *vecs, uint32_t nq, uint32_t k, int metric, uint32_t flags,
                uint32_t *ids_out, float *scores_out, uint64_t *recall_out, double *seconds_out) {
    return nearest_run_on(c, c->d_X[c->cur], c->D, qids, all, vecs, nq, k, metric, flags, ids_out, scores_out, recall_out, seconds_out, nullptr);
}

// Do the CSR's column ids ascend inside every row?  Checked once per handle, on the host copy.
bool rows_ascending(f2v_ctx *c) {
    if (c->rows_sorted < 0) {
        c->rows_sorted = 1;
        for (uint32_t r = 0; r < c->n && c->rows_sorted; r++)
            for (uint32_t p = c->rowptr[r] + 1; p < c->rowptr[r + 1]; p++)
                if (c->colids[p] < c->colids[p - 1]) { c->rows_sorted = 0; break; }
    }
    return c->rows_sorted == 1;
}

// The entry points' common argument checks, then settled_enter.  -> 1: nq == 0, nothing to do and nothing touched.
// `by_row`: the call searches CSR rows (EXCLUDE_NEIGHBOURS, the recall count), which needs their ids ascending -- f2v_create documents
// that order but no earlier kernel depended on it, so it is verified here, once per handle, on the host copy.
int nearest_enter(f2v_ctx *c, const char *who, uint32_t nq, uint32_t k, int metric, uint32_t flags, bool by_row) {
    if (c->n >= 0xFFFFFFFFu - kNnTile) return fail(F2V_EINVAL, "%s: too many vertices for 32-bit candidate tiles", who);
    if (k == 0 || k > F2V_NEAREST_MAX_K) return fail(F2V_EINVAL, "%s: k = %u is outside 1..%d", who, k, F2V_NEAREST_MAX_K);
    if (metric != F2V_SIM_DOT && metric != F2V_SIM_L2 && metric != F2V_SIM_COSINE) return fail(F2V_EINVAL, "%s: unknown metric %d", who, metric);
    if (flags & ~(F2V_NEAREST_EXCLUDE_SELF | F2V_NEAREST_EXCLUDE_NEIGHBOURS)) return fail(F2V_EINVAL, "%s: unknown flag in 0x%x", who, flags);
    if (by_row) {
        if (!rows_ascending(c)) return fail(F2V_EINVAL, "%s: the CSR's column ids are not ascending inside every row (needed to search a row)", who);
    }
    if (nq == 0 && c->have_x) return 1;
    return settled_enter(c, who);
}

// ---- clustering (f2v_kmeans.hip.h; definition in include/f2v.h) ------------------------------------------------------------------
template <int RB>
int launch_assign_t(f2v_ctx *c, const KmAssignArgs &a) {
    const size_t lds = km_lds_bytes(RB, a.D, a.tile);
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&kmeans_assign_kernel<RB>), lds));
    hipLaunchKernelGGL((kmeans_assign_kernel<RB>), dim3((a.n + RB - 1) / RB), dim3(kKmThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// the workspace of f2v_kmeans for `k` clusters (f2v.h states its size): the per-vertex arrays once, the per-cluster ones for the largest k so far
int kmeans_workspace(f2v_ctx *c, uint32_t k) {
    f2v_ctx::Kmeans &w = c->km;
    const char *what = "clustering";
    const size_t n = c->n, D = c->D, blocks = (n + kKmSortBlock - 1) / kKmSortBlock;
    F2VC(w.d_labels.reserve(c, n, what));
    F2VC(w.d_bestL.reserve(c, n, what));
    F2VC(w.d_order.reserve(c, n, what));
    F2VC(w.d_dist.reserve(c, n, what));
    F2VC(w.d_ipart.reserve(c, (n + kKmPiece - 1) / kKmPiece, what));
    F2VC(w.d_inertia.reserve(c, 1, what));
    F2VC(w.d_changed.reserve(c, 1, what));
    F2VC(w.d_C.reserve(c, k * D, what));
    F2VC(w.d_bestC.reserve(c, k * D, what));
    F2VC(w.d_hist.reserve(c, blocks * k, what));
    F2VC(w.d_counts.reserve(c, k, what));
    F2VC(w.d_start.reserve(c, (size_t)k + 1, what));
    F2VC(w.d_pstart.reserve(c, (size_t)k + 1, what));
    F2VC(w.d_seed.reserve(c, k, what));
    F2VC(w.d_psum.reserve(c, (n / kKmPiece + k) * D, what));
    return F2V_OK;
}

// the k vertices of smallest key(v) = mix64(mix64(seed) ^ v), ties by id, in that order: a bounded heap over one pass
void kmeans_seed_rows(uint32_t n, uint32_t k, uint64_t seed, std::vector<uint32_t> &ids) {
    typedef std::pair<uint64_t, uint32_t> Entry;
    const uint64_t sm = mix64_host(seed);
    std::vector<Entry> heap;
    heap.reserve(k);
    for (uint32_t v = 0; v < n; v++) {
        const Entry e(mix64_host(sm ^ (uint64_t)v), v);
        if (heap.size() < k) {
            heap.push_back(e);
            std::push_heap(heap.begin(), heap.end());
        } else if (e < heap.front()) {
            std::pop_heap(heap.begin(), heap.end());
            heap.back() = e;
            std::push_heap(heap.begin(), heap.end());
        }
    }
    std::sort_heap(heap.begin(), heap.end());
    ids.resize(k);
    for (uint32_t i = 0; i < k; i++) ids[i] = heap[i].second;
}

// histogram, scan: d_counts / d_start / d_pstart of the `m` labels and the per-block offsets the scatter needs
void kmeans_count(f2v_ctx *c, const uint32_t *labels, uint32_t m, uint32_t k) {
    f2v_ctx::Kmeans &w = c->km;
    const uint32_t blocks = (m + kKmSortBlock - 1) / kKmSortBlock;
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3(blocks), dim3(256), 0, c->stream, labels, m, k, w.d_hist);
    hipLaunchKernelGGL(kmeans_offsets_kernel, dim3(k), dim3(256), 0, c->stream, w.d_hist, blocks, k, w.d_counts);
    hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(256), 0, c->stream, (const uint32_t *)w.d_counts, k, w.d_start, w.d_pstart);
}

// ... and the scatter: d_order = the places 0 .. m-1 by (label, place)
void kmeans_sort(f2v_ctx *c, const uint32_t *labels, uint32_t m, uint32_t k) {
    f2v_ctx::Kmeans &w = c->km;
    kmeans_count(c, labels, m, k);
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((m + kKmSortBlock - 1) / kKmSortBlock), dim3(64), 0, c->stream, labels, m, k, (const uint32_t *)w.d_hist,
                       (const uint32_t *)w.d_start, w.d_order);
}

// the arguments of kmeans_piece_sum_kernel over the sorted members
KmSumArgs km_sum_args(f2v_ctx *c, uint32_t k) {
    f2v_ctx::Kmeans &w = c->km;
    KmSumArgs s{};
    s.X = c->d_X[c->cur];
    s.order = w.d_order;
    s.start = w.d_start;
    s.counts = w.d_counts;
    s.pstart = w.d_pstart;
    s.psum = w.d_psum;
    s.n = c->n;
    s.D = c->D;
    s.k = k;
    s.lanes = 1;
    while (s.lanes < 64 && 4 * s.lanes < c->D) s.lanes *= 2;
    return s;
}

// One run of the iteration of f2v.h from the centroids in d_C: leaves L_t in d_labels, C_(t-1) in d_C, the distances in d_dist.
int kmeans_run(f2v_ctx *c, uint32_t k, uint32_t max_iters, uint32_t *iterations, uint32_t *converged) {
    f2v_ctx::Kmeans &w = c->km;
    const uint32_t n = c->n, D = c->D;
    const uint32_t rb = w.block ? w.block : k <= 2 ? 256u : k <= 4 ? 128u : 64u;
    KmAssignArgs a{};
    a.X = c->d_X[c->cur];
    a.C = w.d_C;
    a.labels = w.d_labels;
    a.dist = w.d_dist;
    a.changed = w.d_changed;
    a.n = n;
    a.D = D;
    a.k = k;
    a.tile = km_tile(rb, D, k);
    const KmSumArgs s = km_sum_args(c, k);
    const size_t max_pieces = (size_t)n / kKmPiece + k;
    HIPC(hipMemsetAsync(w.d_labels, 0xFF, (size_t)n * sizeof(uint32_t), c->stream));  // no label yet: the first assignment changes every row
    for (uint32_t t = 1;; t++) {
        HIPC(hipMemsetAsync(w.d_changed, 0, sizeof(uint32_t), c->stream));
        F2VC(rb == 256 ? launch_assign_t<256>(c, a) : rb == 128 ? launch_assign_t<128>(c, a) : launch_assign_t<64>(c, a));
        uint32_t changed = 0;
        HIPC(hipMemcpyAsync(&changed, w.d_changed, sizeof changed, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        if (t > 1 && changed == 0) {
            *iterations = t - 1;
            *converged = 1;
            return F2V_OK;
        }
        if (t - 1 == max_iters) {
            *iterations = max_iters;
            *converged = 0;
            return F2V_OK;
        }
        kmeans_sort(c, w.d_labels, n, k);
        hipLaunchKernelGGL(kmeans_piece_sum_kernel, dim3((uint32_t)((max_pieces * s.lanes + kKmThreads - 1) / kKmThreads)), dim3(kKmThreads), 0, c->stream, s);
        hipLaunchKernelGGL(kmeans_centroid_kernel, dim3(k, (D + 31) / 32), dim3(kKmThreads), 0, c->stream, (const double *)w.d_psum, (const uint32_t *)w.d_counts,
                           (const uint32_t *)w.d_pstart, D, w.d_C);
        HIPC(hipGetLastError());
    }
}

// ---- nearest neighbours through an index (f2v_index.hip.h; definition in include/f2v.h) ------------------------------------------
constexpr size_t kIxMaxKeys = (size_t)1 << 24;  // keys of one launch's result lists (128 MiB): a search runs fewer queries per launch to stay below
constexpr uint32_t kIxMaxSplits = 16;           // candidate ranges of the longest list: bounds the lists the merge reads per query
constexpr uint32_t kIxFewSplits = 2;            // ... in a call of kIxManyPairs (query, list) pairs or more
constexpr uint64_t kIxManyPairs = 16384;

void index_drop(f2v_ctx *c) {
    f2v_ctx::Index &w = c->ix;
    (void)hipStreamSynchronize(c->stream);  // a search may still read it
    w.d_labels.release();
    w.d_members.release();
    w.d_offsets.release();
    w.d_C.release();
    w.offsets.clear();
    w.info = f2v_index_t{};
    w.built = false;
}

// Both builds end here: the host's labels and centroids become the handle's index.  The counting sort into list order (ascending id
// inside a list) is the clustering's own, run in its workspace; what it leaves is copied into the index's buffers.
int index_install(f2v_ctx *c, const char *who, const uint32_t *labels, const float *centroids, uint32_t lists, const f2v_kmeans_t *km, f2v_index_t *info_out) {
    f2v_ctx::Index &w = c->ix;
    const uint32_t n = c->n, D = c->D;
    for (uint32_t v = 0; v < n; v++)
        if (labels[v] >= lists) return fail(F2V_EINVAL, "%s: labels[%u] = %u is not a list (lists = %u)", who, v, labels[v], lists);
    HIPC(hipSetDevice(c->device));
    const char *what = "index";
    w.built = false;
    F2VC(w.d_labels.reserve(c, n, what));
    F2VC(w.d_members.reserve(c, n, what));
    F2VC(w.d_offsets.reserve(c, (size_t)lists + 1, what));
    F2VC(w.d_C.reserve(c, (size_t)lists * D, what));
    F2VC(kmeans_workspace(c, lists));
    HIPC(hipMemcpyAsync(w.d_labels, labels, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_C, centroids, (size_t)lists * D * sizeof(float), hipMemcpyHostToDevice, c->stream));
    F2VC(w.timer.start(c->stream));
    kmeans_sort(c, w.d_labels, n, lists);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(w.d_members, c->km.d_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_offsets, c->km.d_start, ((size_t)lists + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    F2VC(w.timer.stop(c->stream));
    w.offsets.assign((size_t)lists + 1, 0);
    HIPC(hipMemcpyAsync(w.offsets.data(), w.d_offsets, ((size_t)lists + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, who));
    f2v_index_t info{};
    if (km) {
        info.inertia = km->inertia;
        info.seconds = km->seconds;
        info.iterations = km->iterations;
        info.converged = km->converged;
    }
    F2VC(w.timer.seconds(&info.seconds));
    info.bytes = (2 * (uint64_t)n + lists + 1) * sizeof(uint32_t) + (uint64_t)lists * D * sizeof(float);
    info.lists = lists;
    for (uint32_t l = 0; l < lists; l++) {
        const uint32_t len = w.offsets[l + 1] - w.offsets[l];
        info.largest = std::max(info.largest, len);
        info.empty += len == 0 ? 1u : 0u;
    }
    w.info = info;
    w.built = true;
    if (info_out) *info_out = info;
    return F2V_OK;
}

template <bool L2, int WQ, int MI, int NI>
int launch_index_scan_t(f2v_ctx *c, const IxArgs &a, uint32_t items) {
    const size_t lds = ix_lds_bytes(32u * WQ * MI, a.D);
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&index_scan_kernel<L2, WQ, MI, NI>), lds));
    hipLaunchKernelGGL((index_scan_kernel<L2, WQ, MI, NI>), dim3(items), dim3(kNnThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// What the two searches share behind their checks.  Queries are rows `qids` of the matrix or the host vectors `vecs`; they run in
// chunks, each chunk as: stage the vectors / rank the centroids (nearest_run_on over the centroid matrix: the defined probe order) /
// count the pairs per list -- the counts come back, the host cuts the buckets into work items -- / fill the buckets / scan / merge.
int index_search(f2v_ctx *c, const char *who, const uint32_t *qids, const float *vecs, uint32_t nq, uint32_t k, int metric, uint32_t flags,
                 uint32_t nprobe, uint32_t *ids_out, float *scores_out, uint32_t *probes_out, f2v_index_search_t *info_out) {
    f2v_ctx::Index &w = c->ix;
    const uint32_t n = c->n, D = c->D, lists = w.info.lists, P = std::min(nprobe, lists);
    const bool rows = qids != nullptr, cosine = metric == F2V_SIM_COSINE;
    const float *X = c->d_X[c->cur];
    const char *what = "index search";
    // candidate ranges per list: placement only (a query's lists are merged whatever their number)
    const uint32_t tiles_max = (w.info.largest + kNnTile - 1) / kNnTile;
    const uint32_t max_splits = (uint64_t)nq * P >= kIxManyPairs ? kIxFewSplits : kIxMaxSplits;  // many pairs fill the card by themselves
    uint32_t tps = w.split_tiles, splits = std::max(1u, (tiles_max + tps - 1) / tps);
    if (splits > max_splits) {
        tps = (tiles_max + max_splits - 1) / max_splits;
        splits = (tiles_max + tps - 1) / tps;
    }
    const uint32_t big = w.block == kIxBlock || D > 128 ? 0u : kIxBlockBig;  // "index_block": the large form's block, 0 where only the small form runs
    const size_t per_query = (size_t)P * splits * k;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(w.chunk, kIxMaxKeys / per_query));
    if (cosine) F2VC(w.d_rc.reserve(c, n, what));
    F2VC(w.d_counts.reserve(c, 2 * (size_t)lists, what));  // the counts, then the fill's cursors
    F2VC(w.d_start.reserve(c, lists, what));
    std::vector<uint32_t> counts(lists), start(lists);
    std::vector<IxItem> items, items_big;
    double seconds = 0.0;
    uint64_t candidates = 0;
    for (uint32_t done = 0; done < nq; done += chunk) {
        const uint32_t cq = std::min(chunk, nq - done), pairs = cq * P;
        const size_t slots = (size_t)cq * k;
        F2VC(w.d_Q.reserve(c, (size_t)cq * D, what));
        F2VC(w.d_rq.reserve(c, cq, what));
        F2VC(w.d_qids.reserve(c, cq, what));
        F2VC(w.d_probes.reserve(c, pairs, what));
        F2VC(w.d_bucket.reserve(c, pairs, what));
        F2VC(w.d_ws.reserve(c, cq * per_query, what));
        F2VC(w.d_ids.reserve(c, slots, what));
        F2VC(w.d_scores.reserve(c, slots, what));
        if (rows) HIPC(hipMemcpyAsync(w.d_qids, qids + done, (size_t)cq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        else HIPC(hipMemcpyAsync(w.d_Q, vecs + (size_t)done * D, (size_t)cq * D * sizeof(float), hipMemcpyHostToDevice, c->stream));
        F2VC(w.timer.start(c->stream));
        if (rows) hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)cq * D + 255) / 256, 4096)), dim3(256), 0, c->stream, X, (const uint32_t *)w.d_qids, cq, D, w.d_Q);
        if (cosine) {
            if (done == 0) hipLaunchKernelGGL(nearest_rnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, X, n, D, w.d_rc);
            hipLaunchKernelGGL(nearest_rnorm_kernel, dim3((cq + 255) / 256), dim3(256), 0, c->stream, (const float *)w.d_Q, cq, D, w.d_rq);
        }
        HIPC(hipGetLastError());
        double probe_seconds = 0.0;  // (inside this call's own events)
        F2VC(nearest_run_on(c, w.d_C, D, nullptr, false, w.d_Q, cq, P, metric, 0, nullptr, nullptr, nullptr, &probe_seconds, w.d_probes, nullptr, lists, true));
        HIPC(hipMemsetAsync(w.d_counts, 0, 2 * (size_t)lists * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(index_count_kernel, dim3((pairs + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)w.d_probes, pairs, lists, w.d_counts);
        HIPC(hipGetLastError());
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(counts.data(), w.d_counts, (size_t)lists * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (probes_out) HIPC(hipMemcpyAsync(probes_out + (size_t)done * P, w.d_probes, (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
        // the work items: per list its bucket in blocks of queries -- 128 where more than 32 are left and the large form runs, else 32 --
        // times its candidate ranges
        items.clear();
        items_big.clear();
        const uint64_t step = (uint64_t)tps * kNnTile;
        uint32_t run = 0;
        for (uint32_t l = 0; l < lists; l++) {
            const uint32_t lo = w.offsets[l], len = w.offsets[l + 1] - lo;
            start[l] = run;
            candidates += (uint64_t)counts[l] * len;
            for (uint32_t b = 0; len && b < counts[l];) {
                const bool large = big && counts[l] - b > kIxBlock;
                const uint32_t qb = large ? big : kIxBlock, cnt = std::min(qb, counts[l] - b);
                for (uint32_t s = 0; s * step < len; s++)
                    (large ? items_big : items).push_back(IxItem{(uint32_t)(lo + s * step), (uint32_t)(lo + std::min<uint64_t>(len, (s + 1) * step)), run + b, cnt, s});
                b += cnt;
            }
            run += counts[l];
        }
        const size_t n_small = items.size(), n_big = items_big.size();
        items.insert(items.end(), items_big.begin(), items_big.end());
        F2VC(w.d_items.reserve(c, items.size(), what));
        HIPC(hipMemcpyAsync(w.d_start, start.data(), (size_t)lists * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (!items.empty()) HIPC(hipMemcpyAsync(w.d_items, items.data(), items.size() * sizeof(IxItem), hipMemcpyHostToDevice, c->stream));
        F2VC(w.timer.start(c->stream));
        HIPC(hipMemsetAsync(w.d_ws, 0, cq * per_query * sizeof(nn_key_t), c->stream));
        hipLaunchKernelGGL(index_fill_kernel, dim3((pairs + 255) / 256), dim3(256), 0, c->stream, (const uint32_t *)w.d_probes, pairs, lists, (const uint32_t *)w.d_start,
                           w.d_counts + lists, w.d_bucket);
        HIPC(hipGetLastError());
        if (!items.empty()) {
            IxArgs a{};
            a.X = X;
            a.Q = w.d_Q;
            a.rq = cosine ? w.d_rq : nullptr;
            a.rc = cosine ? w.d_rc : nullptr;
            a.qids = rows ? w.d_qids : nullptr;
            a.rowptr = c->d_rowptr;
            a.colids = c->d_colids;
            a.members = w.d_members;
            a.bucket = w.d_bucket;
            a.items = w.d_items;
            a.ws = w.d_ws;
            a.n = n;
            a.D = D;
            a.nq = cq;
            a.k = k;
            a.flags = flags;
            a.P = P;
            a.splits = splits;
            a.cosine = cosine ? 1u : 0u;
            if (n_big) {  // first: these are the long work items
                a.items = w.d_items + n_small;
                F2VC((metric == F2V_SIM_L2 ? launch_index_scan_t<true, 2, 2, 2>(c, a, (uint32_t)n_big) : launch_index_scan_t<false, 2, 2, 2>(c, a, (uint32_t)n_big)));
            }
            if (n_small) {
                a.items = w.d_items;
                F2VC((metric == F2V_SIM_L2 ? launch_index_scan_t<true, 1, 1, 1>(c, a, (uint32_t)n_small) : launch_index_scan_t<false, 1, 1, 1>(c, a, (uint32_t)n_small)));
            }
        }
        hipLaunchKernelGGL(nearest_merge_kernel, dim3(cq), dim3(256), 0, c->stream, (const nn_key_t *)w.d_ws, P * splits, k, w.d_ids, w.d_scores);
        HIPC(hipGetLastError());
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(ids_out + (size_t)done * k, w.d_ids, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (scores_out) HIPC(hipMemcpyAsync(scores_out + (size_t)done * k, w.d_scores, slots * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    F2VC(check_kernel_err(c, who));
    if (info_out) *info_out = f2v_index_search_t{seconds, candidates, P, 0};
    return F2V_OK;
}

// The searches' common checks, in the order f2v.h lists them.  -> 1: nq == 0, nothing to do and nothing touched.
int index_enter(f2v_ctx *c, const char *who, uint32_t nq, uint32_t k, int metric, uint32_t flags, uint32_t nprobe, f2v_index_search_t *info_out) {
    if (nprobe == 0 || nprobe > F2V_INDEX_MAX_PROBES) return fail(F2V_EINVAL, "%s: nprobe = %u is outside 1..%d", who, nprobe, F2V_INDEX_MAX_PROBES);
    if (!c->ix.built) return fail(F2V_ESTATE, "%s: the handle has no index: build one first", who);
    const int rc = nearest_enter(c, who, nq, k, metric, flags, (flags & F2V_NEAREST_EXCLUDE_NEIGHBOURS) != 0);
    if (rc == 1 && info_out) *info_out = f2v_index_search_t{0.0, 0, std::min(nprobe, c->ix.info.lists), 0};
    return rc;
}

// ---- logistic regression (f2v_logreg.hip.h; definition in include/f2v.h) ----------------------------------------------------------
constexpr uint32_t kLrDecisionChunk = 262144;  // samples per launch of f2v_logreg_decision: bounds its z buffer

template <bool EVAL, int NA, int NZ>
int launch_logreg_t(f2v_ctx *c, const LrArgs &a) {
    const size_t lds = lr_lds_bytes(a.D, a.cg);
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&logreg_kernel<EVAL, NA, NZ>), lds));
    hipLaunchKernelGGL((logreg_kernel<EVAL, NA, NZ>), dim3((a.m + kLrBlock - 1) / kLrBlock, (a.nc + a.cg - 1) / a.cg), dim3(kLrThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// The instantiation for the call's class group: NZ logits per thread hold 8 NZ classes, NA gradient sums per thread hold 256 NA slots of
// classes x Dp (Dp: the power of two that holds D).  4 NZ sums serve D <= 128; twice and four times as many D <= 256 and D <= 512,
// where lr_group admits 32 and 16 classes.
int launch_logreg(f2v_ctx *c, const LrArgs &a, bool eval) {
    uint32_t nz = 1;
    while (nz * kLrGroups < a.cg) nz *= 2;
    const uint32_t wide = a.lg > 7 ? a.lg - 7 : 0;
    if (!eval) return nz == 1 ? launch_logreg_t<false, 1, 1>(c, a) : nz == 2 ? launch_logreg_t<false, 1, 2>(c, a) : nz == 4 ? launch_logreg_t<false, 1, 4>(c, a)
                                                                                                                            : launch_logreg_t<false, 1, 8>(c, a);
    switch (nz << (4 * wide)) {
    case 0x001: return launch_logreg_t<true, 4, 1>(c, a);
    case 0x002: return launch_logreg_t<true, 8, 2>(c, a);
    case 0x004: return launch_logreg_t<true, 16, 4>(c, a);
    case 0x008: return launch_logreg_t<true, 32, 8>(c, a);
    case 0x010: return launch_logreg_t<true, 8, 1>(c, a);
    case 0x020: return launch_logreg_t<true, 16, 2>(c, a);
    case 0x040: return launch_logreg_t<true, 32, 4>(c, a);
    case 0x100: return launch_logreg_t<true, 16, 1>(c, a);
    case 0x200: return launch_logreg_t<true, 32, 2>(c, a);
    }
    return fail(F2V_EINVAL, "logistic regression: no kernel for %u classes per workgroup at dim %u", a.cg, a.D);
}

// The entry points' common checks and the upload of the samples (and targets).  On success the ids are in lr.d_a / lr.d_b.
int logreg_enter(f2v_ctx *c, const char *who, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const uint8_t *y, uint32_t classes) {
    if (m == 0) return fail(F2V_EINVAL, "%s: m = 0 samples", who);
    if (m > 0xFFFFFFFFu - kLrBlock) return fail(F2V_EINVAL, "%s: too many samples for 32-bit sample blocks", who);
    if (classes == 0 || classes > F2V_LOGREG_MAX_CLASSES) return fail(F2V_EINVAL, "%s: classes = %u is outside 1..%d", who, classes, F2V_LOGREG_MAX_CLASSES);
    if (b_ids && (feature < F2V_PAIR_HADAMARD || feature > F2V_PAIR_AVERAGE)) return fail(F2V_EINVAL, "%s: unknown pair feature %d", who, feature);
    for (uint32_t i = 0; i < m; i++)
        if (a_ids[i] >= c->n || (b_ids && b_ids[i] >= c->n))
            return fail(F2V_EINVAL, "%s: sample %u names vertex %u of %u", who, i, a_ids[i] >= c->n ? a_ids[i] : b_ids[i], c->n);
    const size_t ybytes = (size_t)m * classes;
    for (size_t i = 0; y && i < ybytes; i++)
        if (y[i] > 1) return fail(F2V_EINVAL, "%s: target %zu of sample %zu is %u, not 0 or 1", who, i % classes, i / classes, (unsigned)y[i]);
    F2VC(settled_enter(c, who));
    f2v_ctx::Logreg &w = c->lr;
    const char *what = "logistic-regression";
    const size_t E = (size_t)c->D + 2;
    F2VC(w.d_W.reserve(c, (size_t)F2V_LOGREG_MAX_CLASSES * E, what));
    F2VC(w.d_sums.reserve(c, (size_t)F2V_LOGREG_MAX_CLASSES * E, what));
    F2VC(w.d_cmap.reserve(c, F2V_LOGREG_MAX_CLASSES, what));
    F2VC(w.d_a.reserve(c, m, what));
    F2VC(w.d_b.reserve(c, m, what));
    HIPC(hipMemcpyAsync(w.d_a, a_ids, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (b_ids) HIPC(hipMemcpyAsync(w.d_b, b_ids, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (y) {
        F2VC(w.d_y.reserve(c, ybytes, what));
        F2VC(w.d_part.reserve(c, (size_t)((m + kLrBlock - 1) / kLrBlock) * classes * E, what));
        HIPC(hipMemcpyAsync(w.d_y, y, ybytes, hipMemcpyHostToDevice, c->stream));
    }
    return F2V_OK;
}

LrArgs logreg_args(f2v_ctx *c, bool pairs, uint32_t m, int feature, uint32_t nc, uint32_t classes) {
    LrArgs a{};
    a.X = c->d_X[c->cur];
    a.a = c->lr.d_a;
    a.b = pairs ? c->lr.d_b : c->lr.d_a;
    a.y = c->lr.d_y;
    a.cmap = c->lr.d_cmap;
    a.W = c->lr.d_W;
    a.m = m;
    a.D = c->D;
    a.nc = nc;
    a.C = classes;
    a.cg = lr_group(c->D, nc);
    a.lg = lr_log2(c->D);
    a.feature = pairs ? feature : kLrRow;
    return a;
}

// One pass over the uploaded samples: J and its gradient for the nc classes whose target columns are cmap[], at the weights W
// (nc x (D + 1)) -> loss[nc], grad[nc x (D + 1)]; *seconds += the device time of the launches.
int logreg_pass(f2v_ctx *c, bool pairs, uint32_t m, int feature, uint32_t classes, const uint32_t *cmap, uint32_t nc, const double *W, double lambda,
                double *loss, double *grad, double *seconds) {
    f2v_ctx::Logreg &w = c->lr;
    const uint32_t D = c->D, E = D + 2, blocks = (m + kLrBlock - 1) / kLrBlock;
    HIPC(hipMemcpyAsync(w.d_cmap, cmap, (size_t)nc * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_W, W, (size_t)nc * (D + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LrArgs a = logreg_args(c, pairs, m, feature, nc, classes);
    a.out = w.d_part;
    F2VC(w.timer.start(c->stream));
    F2VC(launch_logreg(c, a, true));
    hipLaunchKernelGGL(logreg_reduce_kernel, dim3((nc * E + 255) / 256), dim3(256), 0, c->stream, (const double *)w.d_part, blocks, nc * E, w.d_sums);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    std::vector<double> sums((size_t)nc * E);
    HIPC(hipMemcpyAsync(sums.data(), w.d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(seconds));
    for (uint32_t k = 0; k < nc; k++) {  // the regulariser, as f2v.h orders it
        const double *wk = W + (size_t)k * (D + 1), *sk = sums.data() + (size_t)k * E;
        double q = 0.0;
        for (uint32_t d = 0; d < D; d++) q = std::fma(wk[d], wk[d], q);
        loss[k] = std::fma(0.5 * lambda, q, sk[D + 1]);
        for (uint32_t d = 0; d < D; d++) grad[(size_t)k * (D + 1) + d] = std::fma(lambda, wk[d], sk[d]);
        grad[(size_t)k * (D + 1) + D] = sk[D];
    }
    return F2V_OK;
}

// ---- the solver of f2v.h: one L-BFGS state per class, plain fp64, sums in ascending order
struct LbfgsClass {
    std::vector<double> w, g, p, trial;
    std::vector<std::vector<double>> S, Y;  // oldest first
    std::vector<double> rho;
    double f = 0.0, t = 0.0, gp = 0.0, gnorm = 0.0;
    uint32_t iterations = 0, evaluations = 0, halvings = 0, converged = 0;
    bool active = true, searching = false;
};

double lr_dot(const std::vector<double> &a, const std::vector<double> &b) {
    double s = 0.0;
    for (size_t i = 0; i < a.size(); i++) s += a[i] * b[i];
    return s;
}

double lr_norm_inf(const std::vector<double> &a) {
    double s = 0.0;
    for (double v : a) s = std::fabs(v) > s || std::isnan(v) ? std::fabs(v) : s;
    return s;
}

// the two-loop recursion -> p = -H g; steepest descent where there is no pair or H g does not descend
void lbfgs_direction(LbfgsClass &k) {
    const size_t n = k.g.size();
    std::vector<double> q = k.g, alpha(k.S.size());
    for (size_t i = k.S.size(); i-- > 0;) {
        alpha[i] = k.rho[i] * lr_dot(k.S[i], q);
        for (size_t j = 0; j < n; j++) q[j] -= alpha[i] * k.Y[i][j];
    }
    if (!k.S.empty()) {
        const double gamma = lr_dot(k.S.back(), k.Y.back()) / lr_dot(k.Y.back(), k.Y.back());
        for (size_t j = 0; j < n; j++) q[j] *= gamma;
    }
    for (size_t i = 0; i < k.S.size(); i++) {
        const double beta = k.rho[i] * lr_dot(k.Y[i], q);
        for (size_t j = 0; j < n; j++) q[j] += k.S[i][j] * (alpha[i] - beta);
    }
    k.p.resize(n);
    for (size_t j = 0; j < n; j++) k.p[j] = -q[j];
    k.gp = lr_dot(k.g, k.p);
    if (!(k.gp < 0.0)) {
        k.S.clear();
        k.Y.clear();
        k.rho.clear();
        for (size_t j = 0; j < n; j++) k.p[j] = -k.g[j];
        k.gp = lr_dot(k.g, k.p);
    }
}

// ---- separation (f2v_separation.hip.h; definition in include/f2v.h) ----------------------------------------------------------------
// What both scores share: the labelling checked, the labelled vertices (ascending id), the member counts
struct SepLabels {
    std::vector<uint32_t> ids, lab, counts;  // the labelled vertices, their labels, members per cluster
    uint32_t nonempty = 0;
};

int sep_check(f2v_ctx *c, const char *who, const uint32_t *labels, uint32_t n_clusters, SepLabels &L) {
    if (n_clusters == 0 || n_clusters > F2V_SEPARATION_MAX_CLUSTERS)
        return fail(F2V_EINVAL, "%s: n_clusters = %u is outside 1..%d", who, n_clusters, F2V_SEPARATION_MAX_CLUSTERS);
    L.counts.assign(n_clusters, 0);
    for (uint32_t v = 0; v < c->n; v++) {
        if (labels[v] == F2V_LABEL_NONE) continue;
        if (labels[v] >= n_clusters) return fail(F2V_EINVAL, "%s: labels[%u] = %u is neither below n_clusters = %u nor F2V_LABEL_NONE", who, v, labels[v], n_clusters);
        L.ids.push_back(v);
        L.lab.push_back(labels[v]);
        L.counts[labels[v]]++;
    }
    for (uint32_t k = 0; k < n_clusters; k++) L.nonempty += L.counts[k] != 0;
    if (L.nonempty < 2) return fail(F2V_EINVAL, "%s: the labelling has %u non-empty clusters, two are needed", who, L.nonempty);
    return F2V_OK;
}

// The state checks, the pending minibatches, the clustering workspace, and the members in cluster order: km.d_order holds the
// labelled vertices by (label, id), km.d_counts / d_start / d_pstart their counts, starts and first pieces.  The counting sort of
// f2v_kmeans.hip.h runs over the labelled vertices' places (a vertex without a label is simply not there) and separation_ids_kernel
// turns the places into vertex ids.
int sep_enter(f2v_ctx *c, const char *who, const SepLabels &L, uint32_t k) {
    if (c->n >= 0xFFFFFFFFu - 256u) return fail(F2V_EINVAL, "%s: too many vertices for 32-bit row blocks", who);
    F2VC(settled_enter(c, who));
    F2VC(kmeans_workspace(c, k));
    f2v_ctx::Kmeans &w = c->km;
    f2v_ctx::Separation &sp = c->sep;
    const uint32_t m = (uint32_t)L.ids.size();
    F2VC(sp.d_ids.reserve(c, m, "separation"));
    HIPC(hipMemcpyAsync(sp.d_ids, L.ids.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_labels, L.lab.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    F2VC(sp.timer.start(c->stream));
    kmeans_sort(c, w.d_labels, m, k);
    hipLaunchKernelGGL(separation_ids_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, w.d_order, (const uint32_t *)sp.d_ids, m);
    HIPC(hipGetLastError());
    return F2V_OK;
}

template <int RB>
int launch_pair_t(f2v_ctx *c, SepPairArgs a, uint32_t spans) {
    a.blocks = (a.nq + RB - 1) / RB;
    hipLaunchKernelGGL((separation_pair_kernel<RB>), dim3(spans * a.blocks), dim3(kSepThreads), 0, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_kmeans(f2v_handle c, uint32_t k, uint32_t max_iters, uint32_t restarts, uint64_t seed, const float *init_centroids, uint32_t *labels_out,
               float *centroids_out, uint64_t *counts_out, f2v_kmeans_t *info_out) {
    if (!c || !labels_out || !info_out) return fail(F2V_EINVAL, "f2v_kmeans: null argument");
    if (k == 0 || k > F2V_KMEANS_MAX_K || k > c->n) return fail(F2V_EINVAL, "f2v_kmeans: k = %u is outside 1..min(%d, n = %u)", k, F2V_KMEANS_MAX_K, c->n);
    if (restarts == 0) return fail(F2V_EINVAL, "f2v_kmeans: restarts must be at least 1");
    if (restarts > 1 && init_centroids) return fail(F2V_EINVAL, "f2v_kmeans: restarts > 1 need seeded centroids (init_centroids must be NULL)");
    if (c->n >= 0xFFFFFFFFu - 256u) return fail(F2V_EINVAL, "f2v_kmeans: too many vertices for 32-bit row blocks");
    F2VC(settled_enter(c, "f2v_kmeans"));
    F2VC(kmeans_workspace(c, k));
    f2v_ctx::Kmeans &w = c->km;
    const uint32_t n = c->n, D = c->D;
    const size_t cbytes = (size_t)k * D * sizeof(float), lbytes = (size_t)n * sizeof(uint32_t);
    f2v_kmeans_t best{};
    std::vector<uint32_t> ids, all_ids;  // every restart's seeded rows, chosen on the host before the timed part
    for (uint32_t r = 0; !init_centroids && r < restarts; r++) {
        kmeans_seed_rows(n, k, seed + r, ids);
        all_ids.insert(all_ids.end(), ids.begin(), ids.end());
    }
    F2VC(w.timer.start(c->stream));
    for (uint32_t r = 0; r < restarts; r++) {
        if (init_centroids) {
            HIPC(hipMemcpyAsync(w.d_C, init_centroids, cbytes, hipMemcpyHostToDevice, c->stream));
        } else {
            HIPC(hipMemcpyAsync(w.d_seed, all_ids.data() + (size_t)r * k, (size_t)k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)k * D + 255) / 256, 4096)), dim3(256), 0, c->stream, (const float *)c->d_X[c->cur],
                               (const uint32_t *)w.d_seed, k, D, w.d_C);
            HIPC(hipGetLastError());
        }
        uint32_t iterations = 0, converged = 0;
        F2VC(kmeans_run(c, k, max_iters, &iterations, &converged));
        const uint32_t parts = (n + kKmPiece - 1) / kKmPiece;
        hipLaunchKernelGGL(kmeans_inertia_piece_kernel, dim3((parts + 255) / 256), dim3(256), 0, c->stream, (const float *)w.d_dist, n, w.d_ipart);
        hipLaunchKernelGGL(kmeans_inertia_reduce_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)w.d_ipart, parts, w.d_inertia);
        HIPC(hipGetLastError());
        double inertia = 0.0;
        HIPC(hipMemcpyAsync(&inertia, w.d_inertia, sizeof inertia, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        if (r == 0 || inertia < best.inertia) {  // (a NaN inertia never replaces a run: ties and NaNs go to the lowest r)
            best.inertia = inertia;
            best.iterations = iterations;
            best.converged = converged;
            best.restart = r;
            if (restarts > 1) {
                HIPC(hipMemcpyAsync(w.d_bestL, w.d_labels, lbytes, hipMemcpyDeviceToDevice, c->stream));
                HIPC(hipMemcpyAsync(w.d_bestC, w.d_C, cbytes, hipMemcpyDeviceToDevice, c->stream));
            }
        }
    }
    const uint32_t *L = restarts > 1 ? w.d_bestL : w.d_labels;
    const float *Cb = restarts > 1 ? w.d_bestC : w.d_C;
    kmeans_count(c, L, n, k);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    std::vector<uint32_t> counts(k);
    HIPC(hipMemcpyAsync(labels_out, L, lbytes, hipMemcpyDeviceToHost, c->stream));
    if (centroids_out) HIPC(hipMemcpyAsync(centroids_out, Cb, cbytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(counts.data(), w.d_counts, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "f2v_kmeans"));
    for (uint32_t i = 0; counts_out && i < k; i++) counts_out[i] = counts[i];
    F2VC(w.timer.seconds(&best.seconds));
    *info_out = best;
    return F2V_OK;
}

int f2v_modularity(f2v_handle c, const uint32_t *labels, uint32_t n_clusters, double *q_out, uint64_t *edges_out, uint64_t *inside_out,
                   uint64_t *degree_out) {
    if (!c || !labels || !q_out) return fail(F2V_EINVAL, "f2v_modularity: null argument");
    if (n_clusters == 0) return fail(F2V_EINVAL, "f2v_modularity: n_clusters must be at least 1");
    for (uint32_t v = 0; v < c->n; v++)
        if (labels[v] >= n_clusters) return fail(F2V_EINVAL, "f2v_modularity: labels[%u] = %u is not below n_clusters = %u", v, labels[v], n_clusters);
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_modularity: the CSR's column ids are not ascending inside every row (needed to search a row)");
    HIPC(hipSetDevice(c->device));
    f2v_ctx::Kmeans &w = c->km;
    const size_t words = 1 + 2 * (size_t)n_clusters;
    F2VC(w.d_mlabels.reserve(c, c->n, "clustering"));
    F2VC(w.d_tallies.reserve(c, words, "clustering"));
    HIPC(hipMemcpyAsync(w.d_mlabels, labels, (size_t)c->n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(w.d_tallies, 0, words * sizeof(unsigned long long), c->stream));
    ModArgs a{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.labels = w.d_mlabels;
    a.tallies = w.d_tallies;
    a.n = c->n;
    a.nc = n_clusters;
    a.lds = n_clusters <= kModLdsClusters && c->nnz < (1ull << 31) ? 1u : 0u;  // a workgroup's 32-bit tallies cannot overflow
    const uint32_t wgs = std::max(1u, std::min((c->n + 3) / 4, 4096u));
    hipLaunchKernelGGL(modularity_kernel, dim3(wgs), dim3(256), a.lds ? 2 * (size_t)n_clusters * sizeof(uint32_t) : 0, c->stream, a);
    HIPC(hipGetLastError());
    std::vector<uint64_t> t(words);
    HIPC(hipMemcpyAsync(t.data(), w.d_tallies, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    const uint64_t m = t[0];
    double q = 0.0;
    for (uint32_t i = 0; m && i < n_clusters; i++) {
        const double x = (double)t[1 + n_clusters + i] / (2.0 * (double)m);
        q += (double)t[1 + i] / (double)m - x * x;
    }
    *q_out = q;
    if (edges_out) *edges_out = m;
    for (uint32_t i = 0; i < n_clusters; i++) {
        if (inside_out) inside_out[i] = t[1 + i];
        if (degree_out) degree_out[i] = t[1 + n_clusters + i];
    }
    return F2V_OK;
}

int f2v_silhouette(f2v_handle c, const uint32_t *labels, uint32_t n_clusters, const uint32_t *sample_ids, uint32_t nq, double *s_out,
                   uint32_t *other_out, double *score_out, double *seconds_out) {
    if (!c || !labels || !score_out) return fail(F2V_EINVAL, "f2v_silhouette: null argument");
    if (sample_ids && nq == 0) return fail(F2V_EINVAL, "f2v_silhouette: nq = 0 samples");
    SepLabels L;
    F2VC(sep_check(c, "f2v_silhouette", labels, n_clusters, L));
    if (L.nonempty >= L.ids.size())
        return fail(F2V_EINVAL, "f2v_silhouette: %u non-empty clusters for %zu labelled vertices (at most one fewer is allowed)", L.nonempty, L.ids.size());
    const uint32_t k = n_clusters;
    if (!sample_ids) nq = (uint32_t)L.ids.size();
    const uint32_t *sid = sample_ids ? sample_ids : L.ids.data();
    std::vector<uint32_t> slab(nq);
    for (uint32_t i = 0; i < nq; i++) {
        if (sid[i] >= c->n) return fail(F2V_EINVAL, "f2v_silhouette: sample %u names vertex %u of %u", i, sid[i], c->n);
        if (labels[sid[i]] == F2V_LABEL_NONE) return fail(F2V_EINVAL, "f2v_silhouette: sample %u (vertex %u) has no label", i, sid[i]);
        slab[i] = labels[sid[i]];
    }
    // the spans: cluster by cluster, 4096 members each but a cluster's last
    std::vector<uint32_t> span_start, span_cnt, cspan(k + 1);
    uint32_t run = 0;
    for (uint32_t cl = 0; cl < k; cl++) {
        cspan[cl] = (uint32_t)span_start.size();
        for (uint32_t o = 0; o < L.counts[cl]; o += kSepPiece * kSepSpan) {
            span_start.push_back(run + o);
            span_cnt.push_back(std::min(L.counts[cl] - o, kSepPiece * kSepSpan));
        }
        run += L.counts[cl];
    }
    cspan[k] = (uint32_t)span_start.size();
    const uint32_t spans = cspan[k], chunk = std::min(c->sep.chunk, nq), parts = (nq + kSepPiece - 1) / kSepPiece;
    const uint32_t rb = c->sep.block ? c->sep.block : 64u;
    if ((uint64_t)spans * ((chunk + rb - 1) / rb) > 0x7FFFFFFFull) return fail(F2V_EINVAL, "f2v_silhouette: too many workgroups per launch: lower \"separation_chunk\"");
    F2VC(sep_enter(c, "f2v_silhouette", L, k));
    f2v_ctx::Kmeans &w = c->km;
    f2v_ctx::Separation &sp = c->sep;
    const char *what = "separation";
    F2VC(sp.d_sid.reserve(c, nq, what));
    F2VC(sp.d_slab.reserve(c, nq, what));
    F2VC(sp.d_other.reserve(c, nq, what));
    F2VC(sp.d_s.reserve(c, nq, what));
    F2VC(sp.d_part.reserve(c, parts, what));
    F2VC(sp.d_sum.reserve(c, 1, what));
    F2VC(sp.d_span_start.reserve(c, spans, what));
    F2VC(sp.d_span_cnt.reserve(c, spans, what));
    F2VC(sp.d_cspan.reserve(c, (size_t)k + 1, what));
    F2VC(sp.d_ws.reserve(c, (size_t)spans * chunk, what));
    HIPC(hipMemcpyAsync(sp.d_sid, sid, (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(sp.d_slab, slab.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(sp.d_span_start, span_start.data(), (size_t)spans * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(sp.d_span_cnt, span_cnt.data(), (size_t)spans * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(sp.d_cspan, cspan.data(), ((size_t)k + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cq = std::min(chunk, nq - q0);
        SepPairArgs a{};
        a.X = c->d_X[c->cur];
        a.order = w.d_order;
        a.sid = sp.d_sid + q0;
        a.span_start = sp.d_span_start;
        a.span_cnt = sp.d_span_cnt;
        a.ws = sp.d_ws;
        a.D = c->D;
        a.nq = cq;
        a.chunk = chunk;
        F2VC(rb == 128 ? launch_pair_t<128>(c, a, spans) : launch_pair_t<64>(c, a, spans));
        SepFinishArgs f{};
        f.ws = sp.d_ws;
        f.slab = sp.d_slab + q0;
        f.counts = w.d_counts;
        f.cspan = sp.d_cspan;
        f.s = sp.d_s + q0;
        f.other = sp.d_other + q0;
        f.nq = cq;
        f.chunk = chunk;
        f.k = k;
        hipLaunchKernelGGL(separation_finish_kernel, dim3((cq + 255) / 256), dim3(256), 0, c->stream, f);
        HIPC(hipGetLastError());
    }
    hipLaunchKernelGGL(separation_piece_kernel, dim3((parts + 255) / 256), dim3(256), 0, c->stream, (const double *)sp.d_s, nq, sp.d_part);
    hipLaunchKernelGGL(kmeans_inertia_reduce_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)sp.d_part, parts, sp.d_sum);
    HIPC(hipGetLastError());
    F2VC(sp.timer.stop(c->stream));
    double sum = 0.0, seconds = 0.0;
    HIPC(hipMemcpyAsync(&sum, sp.d_sum, sizeof sum, hipMemcpyDeviceToHost, c->stream));
    if (s_out) HIPC(hipMemcpyAsync(s_out, sp.d_s, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (other_out) HIPC(hipMemcpyAsync(other_out, sp.d_other, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "f2v_silhouette"));
    *score_out = sum / (double)nq;
    F2VC(sp.timer.seconds(&seconds));
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

int f2v_davies_bouldin(f2v_handle c, const uint32_t *labels, uint32_t n_clusters, double *score_out, float *centroids_out, double *scatter_out,
                       uint64_t *counts_out, double *seconds_out) {
    if (!c || !labels || !score_out) return fail(F2V_EINVAL, "f2v_davies_bouldin: null argument");
    SepLabels L;
    F2VC(sep_check(c, "f2v_davies_bouldin", labels, n_clusters, L));
    const uint32_t k = n_clusters, D = c->D;
    F2VC(sep_enter(c, "f2v_davies_bouldin", L, k));
    f2v_ctx::Kmeans &w = c->km;
    f2v_ctx::Separation &sp = c->sep;
    uint32_t pieces = 0;
    for (uint32_t cl = 0; cl < k; cl++) pieces += (L.counts[cl] + kSepPiece - 1) / kSepPiece;
    F2VC(sp.d_part.reserve(c, pieces, "separation"));
    F2VC(sp.d_S.reserve(c, k, "separation"));
    // the centroids: the k-means update of f2v.h (an empty cluster's row stays zero)
    const KmSumArgs s = km_sum_args(c, k);
    HIPC(hipMemsetAsync(w.d_C, 0, (size_t)k * D * sizeof(float), c->stream));
    hipLaunchKernelGGL(kmeans_piece_sum_kernel, dim3((uint32_t)(((size_t)pieces * s.lanes + kKmThreads - 1) / kKmThreads)), dim3(kKmThreads), 0, c->stream, s);
    hipLaunchKernelGGL(kmeans_centroid_kernel, dim3(k, (D + 31) / 32), dim3(kKmThreads), 0, c->stream, (const double *)w.d_psum, (const uint32_t *)w.d_counts,
                       (const uint32_t *)w.d_pstart, D, w.d_C);
    SepScatterArgs a{};
    a.X = s.X;
    a.C = w.d_C;
    a.order = w.d_order;
    a.start = w.d_start;
    a.counts = w.d_counts;
    a.pstart = w.d_pstart;
    a.part = sp.d_part;
    a.D = D;
    a.k = k;
    hipLaunchKernelGGL(separation_scatter_kernel, dim3(pieces), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(separation_cluster_kernel, dim3((k + 63) / 64), dim3(64), 0, c->stream, (const double *)sp.d_part, (const uint32_t *)w.d_counts,
                       (const uint32_t *)w.d_pstart, k, sp.d_S);
    HIPC(hipGetLastError());
    F2VC(sp.timer.stop(c->stream));
    std::vector<float> C((size_t)k * D);
    std::vector<double> S(k);
    HIPC(hipMemcpyAsync(C.data(), w.d_C, C.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(S.data(), sp.d_S, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "f2v_davies_bouldin"));
    // K x K centroid distances and the maxima: small, on the host (this translation unit is built without fast-math and without
    // contraction: fmaf and sqrtf are the single correctly rounded operations of the definition)
    double total = 0.0;
    for (uint32_t ci = 0; ci < k; ci++) {
        if (!L.counts[ci]) continue;
        double mx = 0.0;
        bool first = true;
        for (uint32_t di = 0; di < k; di++) {
            if (di == ci || !L.counts[di]) continue;
            const float *x = C.data() + (size_t)ci * D, *y = C.data() + (size_t)di * D;
            float acc = 0.f;
            for (uint32_t d = 0; d < D; d++) {
                const float t = x[d] - y[d];
                acc = std::fmaf(t, t, acc);
            }
            const double M = (double)std::sqrt(acc), ss = S[ci] + S[di];
            const double R = ss == 0.0 ? 0.0 : ss / M;
            if (first || R > mx) mx = R;
            first = false;
        }
        total += mx;
    }
    *score_out = total / (double)L.nonempty;
    if (centroids_out) memcpy(centroids_out, C.data(), C.size() * sizeof(float));
    for (uint32_t i = 0; i < k; i++) {
        if (scatter_out) scatter_out[i] = S[i];
        if (counts_out) counts_out[i] = L.counts[i];
    }
    double seconds = 0.0;
    F2VC(sp.timer.seconds(&seconds));
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

}  // extern "C"

// ---- fold-in (f2v_foldin.hip.h; definition in include/f2v.h) ---------------------------------------------------------------------
namespace {

int launch_fold_q(f2v_ctx *c, int math, uint32_t width, const FoldArgs &a, uint32_t blocks, size_t lds) {
    const uint32_t threads = 64u * (uint32_t)c->waves_per_block;
    F2VC((dispatch_subwave<16, false>(c, math, width, [&](auto O, auto L, auto N, auto, auto FL) {
        hipLaunchKernelGGL((fold_q_kernel<decltype(O)::value, decltype(L)::value, decltype(N)::value, decltype(FL)::value>), dim3(blocks), dim3(threads), lds,
                           c->stream, a);
    })));
    HIPC(hipGetLastError());
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_fold_in(f2v_handle c, int option, const uint32_t *q_rowptr, const uint32_t *q_colids, uint32_t m, uint32_t iters, uint32_t ns, float lr, int init_kind,
                const float *init, uint64_t seed, uint64_t index_base, float *y_out, f2v_fold_t *info) {
    if (!c) return fail(F2V_EINVAL, "f2v_fold_in: null argument");
    const int math = math_of_option(option);
    if (math != 5 && math != 6) return fail(F2V_EINVAL, "f2v_fold_in: option %d (options 5, 8, 11 and 6, 9 fold in)", option);
    if (init_kind != F2V_FOLD_INIT_MEAN && init_kind != F2V_FOLD_INIT_RANDOM && init_kind != F2V_FOLD_INIT_GIVEN)
        return fail(F2V_EINVAL, "f2v_fold_in: unknown init_kind %d", init_kind);
    if (init_kind == F2V_FOLD_INIT_GIVEN && !init && m) return fail(F2V_EINVAL, "f2v_fold_in: F2V_FOLD_INIT_GIVEN without init");
    if (c->n < 1) return fail(F2V_EINVAL, "f2v_fold_in: no vertex to sample");
    const unsigned __int128 counters = ((unsigned __int128)index_base + m) * iters, counter_limit = (unsigned __int128)1 << 62;
    if (ns != 0 && (counters >= counter_limit || counters * ns >= counter_limit))
        return fail(F2V_EINVAL, "f2v_fold_in: (index_base + m) * iters * ns reaches 2^62");
    if (info) *info = f2v_fold_t{};
    if (m == 0 && c->have_x) return F2V_OK;
    if (m && (!q_rowptr || !y_out)) return fail(F2V_EINVAL, "f2v_fold_in: null argument");
    for (uint32_t q = 0; q < m; q++)
        if (q_rowptr[q + 1] < q_rowptr[q]) return fail(F2V_EINVAL, "f2v_fold_in: q_rowptr descends at vertex %u", q);
    const uint32_t base = m ? q_rowptr[0] : 0u, total = m ? q_rowptr[m] - base : 0u;
    if (total && !q_colids) return fail(F2V_EINVAL, "f2v_fold_in: null argument");
    for (uint32_t k = 0; k < total; k++)
        if (q_colids[base + k] >= c->n) return fail(F2V_EINVAL, "f2v_fold_in: q_colids[%u] = %u is not one of the %u vertices", base + k, q_colids[base + k], c->n);
    F2VC(settled_enter(c, "f2v_fold_in"));
    if (m == 0) return F2V_OK;

    f2v_ctx::Fold &w = c->fold;
    const uint32_t n = c->n, D = c->D, chunk = std::min(w.chunk, m);
    const uint32_t width = subwave_width(c), wpb = (uint32_t)c->waves_per_block;
    const uint32_t ipb = items_per_wave(width) * wpb;  // vertices per workgroup
    const size_t table_bytes = math == 5 ? 0 : kSmTableSize * sizeof(float);  // the quarter-wave kernel's dynamic LDS: the sigmoid table

    // the lists, rebased to 0; per chunk the vertices by descending list length (stable: placement only, and the same every call)
    std::vector<uint32_t> rowptr(m + 1), order(m);
    for (uint32_t q = 0; q <= m; q++) rowptr[q] = q_rowptr[q] - base;
    uint64_t pairs = 0;
    for (uint32_t q0 = 0; q0 < m; q0 += chunk) {
        const uint32_t cq = std::min(chunk, m - q0);
        uint32_t *o = order.data() + q0;
        for (uint32_t r = 0; r < cq; r++) o[r] = q0 + r;
        std::stable_sort(o, o + cq, [&](uint32_t x, uint32_t y) { return rowptr[x + 1] - rowptr[x] > rowptr[y + 1] - rowptr[y]; });
    }
    for (uint32_t q = 0; q < m; q++) pairs += ((uint64_t)(rowptr[q + 1] - rowptr[q]) + ns) * iters;

    const char *what = "fold-in";
    F2VC(w.d_rowptr.reserve(c, (size_t)m + 1, what));
    F2VC(w.d_ids.reserve(c, total, what));
    F2VC(w.d_order.reserve(c, m, what));
    F2VC(w.d_in.reserve(c, (size_t)chunk * D, what));
    F2VC(w.d_out.reserve(c, (size_t)chunk * D, what));
    HIPC(hipMemcpyAsync(w.d_rowptr, rowptr.data(), ((size_t)m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (total) HIPC(hipMemcpyAsync(w.d_ids, q_colids + base, (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_order, order.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));

    FoldArgs a{};
    a.X = c->d_X[c->cur];
    a.rowptr = w.d_rowptr;
    a.ids = w.d_ids;
    a.Y0 = w.d_in;
    a.Y = w.d_out;
    a.sm_table = c->d_table;
    a.seed_mix = mix64_host(seed);
    a.index_base = index_base;
    a.n = n;
    a.D = D;
    a.iters = iters;
    a.ns = ns;
    a.lr = lr;
    double seconds = 0.0;
    for (uint32_t q0 = 0; q0 < m; q0 += chunk) {
        const uint32_t cq = std::min(chunk, m - q0);
        a.q0 = q0;
        a.count = cq;
        if (init_kind == F2V_FOLD_INIT_GIVEN)
            HIPC(hipMemcpyAsync(w.d_in, init + (size_t)q0 * D, (size_t)cq * D * sizeof(float), hipMemcpyHostToDevice, c->stream));
        F2VC(w.timer.start(c->stream));
        if (init_kind != F2V_FOLD_INIT_GIVEN) {
            hipLaunchKernelGGL(fold_init_kernel, dim3((uint32_t)(((size_t)cq * D + 255) / 256)), dim3(256), 0, c->stream, a, init_kind, math == 5 ? 0 : 1);
            HIPC(hipGetLastError());
        }
        if (iters > 0 && width != 0) {
            a.order = w.d_order + q0;
            F2VC(launch_fold_q(c, math, width, a, (cq + ipb - 1) / ipb, table_bytes));
        } else if (iters > 0) {
            a.order = w.d_order + q0;
            F2VC(dispatch_math_layout(c, math, [&](auto O, auto V, auto E) {
                hipLaunchKernelGGL((fold_kernel<decltype(O)::value, decltype(V)::value, decltype(E)::value>), dim3((cq + wpb - 1) / wpb), dim3(64 * wpb), 0, c->stream, a);
            }));
            HIPC(hipGetLastError());
        }
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(y_out + (size_t)q0 * D, iters > 0 ? w.d_out : w.d_in, (size_t)cq * D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    if (info) {
        info->seconds = seconds;
        info->pairs = pairs;
        info->resident = 0;  // (the form is not built: "fold_resident")
    }
    return F2V_OK;
}

}  // extern "C"

// ---- link prediction pairs (f2v_linkpairs.hip.h; definition in include/f2v.h) ---------------------------------------------------
namespace {

// Which vertices draw negatives, and how: by descending total(u), ties in id order -- the first `nw` with tables in the workspace, up
// to `nl` a workgroup each, the others a wavefront each.  Shared by f2v_link_pairs and f2v_edge_split, each with buffers of its own.
struct LinkPlan {
    std::vector<uint32_t> order;
    uint32_t nw = 0, nl = 0;
};

// placement (a counting sort: total(u) < n / 2); the order and the workspace tables go to the device, a.keys / table_words / table_at are set
int link_place(f2v_ctx *c, const char *who, const char *what, const std::vector<uint32_t> &total, uint32_t short_max, DevBuf<uint32_t> &d_order,
               DevBuf<unsigned long long> &d_table_at, DevBuf<uint32_t> &d_table, LinkArgs &a, LinkPlan &pl) {
    const uint32_t n = c->n;
    uint32_t most = 0;
    for (uint32_t v = 0; v < n; v++) most = std::max(most, total[v]);
    if (most > (1u << 29)) return fail(F2V_EINVAL, "%s: a vertex with more than 2^29 negatives", who);
    std::vector<uint32_t> first((size_t)most + 2, 0), &order = pl.order;
    for (uint32_t v = 0; v < n; v++)
        if (total[v]) first[most - total[v] + 1]++;
    for (uint32_t k = 0; k <= most; k++) first[k + 1] += first[k];
    order.resize(first[(size_t)most + 1]);
    for (uint32_t v = 0; v < n; v++)
        if (total[v]) order[first[most - total[v]]++] = v;
    const uint32_t cnt = (uint32_t)order.size();
    uint32_t nw = 0, nl = 0;
    std::vector<unsigned long long> table_at;
    uint64_t words = 0;
    while (nl < cnt && total[order[nl]] > short_max) nl++;
    while (nw < nl && link_slots(total[order[nw]]) > kLinkLdsSlots) {
        table_at.push_back(words);
        words += link_slots(total[order[nw++]]);
    }
    pl.nw = nw;
    pl.nl = nl;
    F2VC(d_order.reserve(c, cnt, what));
    F2VC(d_table_at.reserve(c, nw, what));
    F2VC(d_table.reserve(c, 2 * words, what));
    if (cnt) HIPC(hipMemcpyAsync(d_order, order.data(), (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (nw) {
        HIPC(hipMemcpyAsync(d_table_at, table_at.data(), (size_t)nw * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemsetAsync(d_table, 0xFF, 2 * words * sizeof(uint32_t), c->stream));  // kLinkEmpty
    }
    a.keys = d_table;
    a.table_words = words;
    a.table_at = d_table_at;
    return F2V_OK;
}

// the launches that draw: every negative goes straight to its place in a.u_out / v_out / y_out
int link_draw(f2v_ctx *c, const std::vector<uint32_t> &total, const LinkPlan &pl, const uint32_t *d_order, LinkArgs &a) {
    const std::vector<uint32_t> &order = pl.order;
    const uint32_t cnt = (uint32_t)order.size(), nw = pl.nw, nl = pl.nl;
    // link_long_kernel: the wavefronts' counts of two rounds, in front of an LDS table
    const size_t counts_bytes = 2 * (kLinkLongThreads / 64) * sizeof(uint32_t), wide_counts_bytes = 2 * (kLinkWideThreads / 64) * sizeof(uint32_t);
    if (nw) {  // the longest lists first: their workgroups run longest
        a.order = d_order;
        hipLaunchKernelGGL(link_long_kernel<true>, dim3(nw), dim3(kLinkWideThreads), wide_counts_bytes, c->stream, a);
    }
    for (uint32_t i = nw, j; i < nl; i = j) {  // one launch per table size
        a.slots = (uint32_t)link_slots(total[order[i]]);
        for (j = i + 1; j < nl && j - i < (1u << 30) && link_slots(total[order[j]]) == a.slots; j++) {}
        const size_t lds = counts_bytes + 2 * (size_t)a.slots * sizeof(uint32_t);
        F2VC(allow_lds(c, reinterpret_cast<const void *>(&link_long_kernel<false>), lds));
        a.order = d_order + i;
        hipLaunchKernelGGL(link_long_kernel<false>, dim3(j - i), dim3(kLinkLongThreads), lds, c->stream, a);
    }
    if (nl < cnt) {
        a.order = d_order + nl;
        a.count = cnt - nl;
        a.short_max = total[order[nl]];  // the longest list of the launch
        hipLaunchKernelGGL(link_short_kernel, dim3(std::min((a.count + 3) / 4, 16384u)), dim3(256), 4 * (size_t)a.short_max * sizeof(uint32_t), c->stream, a);
    }
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_link_pairs(f2v_handle c, uint32_t ratio, uint64_t seed, uint32_t *u_out, uint32_t *v_out, uint8_t *y_out, uint64_t cap, uint64_t *count_out,
                   f2v_link_t *info) {
    if (!c || !count_out) return fail(F2V_EINVAL, "f2v_link_pairs: null argument");
    const bool fill = u_out || v_out || y_out;
    if (fill && !(u_out && v_out && y_out)) return fail(F2V_EINVAL, "f2v_link_pairs: u_out, v_out and y_out are given together or not at all");
    if (ratio < 1 || ratio > 16) return fail(F2V_EINVAL, "f2v_link_pairs: ratio = %u is outside 1..16", ratio);
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_link_pairs: the CSR's column ids are not ascending inside every row (needed to search a row)");
    HIPC(hipSetDevice(c->device));
    *count_out = 0;
    if (info) *info = f2v_link_t{};
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;

    f2v_ctx::Link &w = c->link;
    const char *what = "link pairs";
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kLinkScanTile - 1) / kLinkScanTile), rows = std::min((n + 3) / 4, 8192u);
    F2VC(w.d_p.reserve(c, n, what));
    F2VC(w.d_total.reserve(c, n, what));
    F2VC(w.d_offset.reserve(c, n, what));
    F2VC(w.d_tile.reserve(c, tiles, what));
    F2VC(w.d_sums.reserve(c, 4, what));
    LinkArgs a{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.p = w.d_p;
    a.total = w.d_total;
    a.offset = w.d_offset;
    a.tile = w.d_tile;
    a.sums = w.d_sums;
    a.n = n;
    a.ratio = ratio;
    a.s1 = mix64_host(seed);
    a.s2 = mix64_host(a.s1);
    HIPC(hipMemsetAsync(w.d_sums, 0, 4 * sizeof(unsigned long long), c->stream));
    double seconds = 0.0;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(link_count_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(link_scan_tile_kernel, dim3(tiles), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(link_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, a, tiles);
    hipLaunchKernelGGL(link_scan_apply_kernel, dim3(tiles), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long sums[4];
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint32_t> total(fill ? n : 0);
    if (fill) HIPC(hipMemcpyAsync(total.data(), w.d_total, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    const uint64_t M = sums[0] + sums[1];
    *count_out = M;
    if (info) {
        info->seconds = seconds;
        info->positives = sums[0];
        info->negatives = sums[1];
        info->capped = sums[2];
    }
    if (fill && cap < M) return fail(F2V_EINVAL, "f2v_link_pairs: the set has %llu pairs, the arrays hold %llu", (unsigned long long)M, (unsigned long long)cap);
    if (!fill || M == 0) return F2V_OK;

    LinkPlan plan;
    F2VC(link_place(c, "f2v_link_pairs", what, total, w.short_max, w.d_order, w.d_table_at, w.d_table, a, plan));
    F2VC(w.d_u.reserve(c, M, what));
    F2VC(w.d_v.reserve(c, M, what));
    F2VC(w.d_y.reserve(c, M, what));
    a.u_out = w.d_u;
    a.v_out = w.d_v;
    a.y_out = w.d_y;
    a.M = M;
    uint32_t bits = 2;
    while (bits < 64 && ((uint64_t)1 << bits) < M) bits += 2;
    a.half = bits / 2;
    a.mask = ((uint64_t)1 << a.half) - 1;
    F2VC(w.timer.start(c->stream));
    F2VC(link_draw(c, total, plan, w.d_order, a));
    hipLaunchKernelGGL(link_positive_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    HIPC(hipMemcpyAsync(u_out, w.d_u, M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(v_out, w.d_v, M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(y_out, w.d_y, M * sizeof(uint8_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    if (info) {
        info->seconds = seconds;
        info->candidates = sums[3];
    }
    return F2V_OK;
}

}  // extern "C"

// ---- held-out link prediction (f2v_heldout.hip.h; definition in include/f2v.h) ---------------------------------------------------
namespace {

// the greatest spanning forest of `seed` as one flag per nonzero in c->cc.d_flag (the components section below)
int forest_flags(f2v_ctx *c, const char *who, uint64_t seed, double *seconds);

// f2v_edge_split (`forest` false: the anchors protect) and f2v_edge_split_connected (true: the greatest spanning forest does): one
// definition but for the protection rule, so one body; the anchor path launches what it always launched
int edge_split_impl(f2v_ctx *c, const char *who, bool forest, double frac, uint64_t seed, uint32_t ratio, uint32_t *rowptr_train, uint32_t *colids_train,
                    uint64_t cap_train, uint32_t *held_u, uint32_t *held_v, uint64_t cap_held, uint32_t *neg_u, uint32_t *neg_v, uint64_t cap_neg,
                    uint64_t *train_nnz_out, uint64_t *held_out, uint64_t *negatives_out, f2v_split_t *info) {
    if (!c || !train_nnz_out || !held_out || !negatives_out) return fail(F2V_EINVAL, "%s: null argument", who);
    const int given = (rowptr_train != nullptr) + (colids_train != nullptr) + (held_u != nullptr) + (held_v != nullptr) + (neg_u != nullptr) + (neg_v != nullptr);
    if (given != 0 && given != 6) return fail(F2V_EINVAL, "%s: the six output arrays are given together or not at all", who);
    const bool fill = given == 6;
    if (!(frac >= 0.0 && frac < 1.0)) return fail(F2V_EINVAL, "%s: frac = %g is outside [0, 1)", who, frac);
    if (ratio > 16) return fail(F2V_EINVAL, "%s: ratio = %u is outside 0..16", who, ratio);
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "%s: the CSR's column ids are not ascending inside every row (needed to search a row)", who);
    HIPC(hipSetDevice(c->device));
    *train_nnz_out = *held_out = *negatives_out = 0;
    if (info) *info = f2v_split_t{};
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;

    f2v_ctx::Heldout &w = c->held;
    const char *what = "edge split";
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kLinkScanTile - 1) / kLinkScanTile), rows = std::min((n + 3) / 4, 8192u);
    F2VC(w.d_anchor.reserve(c, n, what));
    F2VC(w.d_kept.reserve(c, n, what));
    F2VC(w.d_q.reserve(c, n, what));
    F2VC(w.d_total.reserve(c, n, what));
    F2VC(w.d_zero.reserve(c, n, what));
    F2VC(w.d_kept_at.reserve(c, n, what));
    F2VC(w.d_held_at.reserve(c, n, what));
    F2VC(w.d_neg_at.reserve(c, n, what));
    F2VC(w.d_tile.reserve(c, tiles, what));
    F2VC(w.d_sums.reserve(c, 12, what));  // [0..5] held_count_kernel's, [8..11] the link kernels' ([11]: candidates drawn)
    const uint64_t s1 = mix64_host(seed);
    HeldArgs a{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.anchor = w.d_anchor;
    a.kept = w.d_kept;
    a.q = w.d_q;
    a.total = w.d_total;
    a.kept_at = w.d_kept_at;
    a.held_at = w.d_held_at;
    a.sums = w.d_sums;
    a.se = mix64_host(s1 ^ 0x65646765ull);
    a.T = (uint64_t)(frac * 18446744073709551616.0);  // exact product, truncating conversion
    a.n = n;
    a.ratio = ratio;
    LinkArgs l{};  // the scans and the negative draws of f2v_linkpairs.hip.h
    l.rowptr = c->d_rowptr;
    l.colids = c->d_colids;
    l.tile = w.d_tile;
    l.sums = w.d_sums + 8;
    l.n = n;
    l.ratio = ratio;
    l.s1 = mix64_host(s1 ^ 0x6e656773ull);  // SN
    l.M = ~0ull;  // half = 0, mask = 0: link_perm is the identity
    HIPC(hipMemsetAsync(w.d_sums, 0, 12 * sizeof(unsigned long long), c->stream));
    HIPC(hipMemsetAsync(w.d_zero, 0, (size_t)n * sizeof(uint32_t), c->stream));
    auto scan = [&](uint32_t *p, uint32_t *total, unsigned long long *offset) {
        l.p = p;
        l.total = total;
        l.offset = offset;
        hipLaunchKernelGGL(link_scan_tile_kernel, dim3(tiles), dim3(256), 0, c->stream, l);
        hipLaunchKernelGGL(link_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, l, tiles);
        hipLaunchKernelGGL(link_scan_apply_kernel, dim3(tiles), dim3(256), 0, c->stream, l);
    };
    double seconds = 0.0;
    if (forest) {
        F2VC(forest_flags(c, who, seed, &seconds));
        a.forest = c->cc.d_flag;
    }
    F2VC(w.timer.start(c->stream));
    if (forest) {
        hipLaunchKernelGGL(held_forest_count_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    } else {
        hipLaunchKernelGGL(held_anchor_kernel, dim3(rows), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL(held_count_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    }
    scan(w.d_kept, w.d_zero, w.d_kept_at);
    scan(w.d_q, w.d_zero, w.d_held_at);
    scan(w.d_zero, w.d_total, w.d_neg_at);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long sums[12];
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint32_t> total(fill ? n : 0);
    if (fill) HIPC(hipMemcpyAsync(total.data(), w.d_total, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    const uint64_t H = sums[2], nnz_train = sums[3], negs = sums[4];
    *train_nnz_out = nnz_train;
    *held_out = H;
    *negatives_out = negs;
    if (info) {
        info->seconds = seconds;
        info->edges = sums[0];
        info->candidates_held = sums[1];
        info->protected_edges = sums[1] - sums[2];
        info->held = H;
        info->train_nnz = nnz_train;
        info->negatives = negs;
        info->capped = sums[5];
    }
    if (fill && (cap_train < nnz_train || cap_held < H || cap_neg < negs))
        return fail(F2V_EINVAL, "%s: %llu training nonzeros, %llu held pairs and %llu negatives; the arrays hold %llu, %llu and %llu", who,
                    (unsigned long long)nnz_train, (unsigned long long)H, (unsigned long long)negs, (unsigned long long)cap_train, (unsigned long long)cap_held,
                    (unsigned long long)cap_neg);
    if (!fill) return F2V_OK;

    F2VC(w.d_rowptr.reserve(c, (size_t)n + 1, what));
    F2VC(w.d_colids.reserve(c, nnz_train, what));
    F2VC(w.d_hu.reserve(c, H, what));
    F2VC(w.d_hv.reserve(c, H, what));
    F2VC(w.d_nu.reserve(c, negs, what));
    F2VC(w.d_nv.reserve(c, negs, what));
    F2VC(w.d_ny.reserve(c, negs, what));
    a.rowptr_out = w.d_rowptr;
    a.colids_out = w.d_colids;
    a.held_u = w.d_hu;
    a.held_v = w.d_hv;
    LinkPlan plan;
    if (negs) {
        F2VC(link_place(c, who, what, total, c->link.short_max, w.d_order, w.d_table_at, w.d_table, l, plan));
        l.p = w.d_zero;
        l.total = w.d_total;
        l.offset = w.d_neg_at;
        l.u_out = w.d_nu;
        l.v_out = w.d_nv;
        l.y_out = w.d_ny;
    }
    F2VC(w.timer.start(c->stream));
    if (forest) hipLaunchKernelGGL(held_forest_fill_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(held_fill_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    if (negs) F2VC(link_draw(c, total, plan, w.d_order, l));
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    HIPC(hipMemcpyAsync(rowptr_train, w.d_rowptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (nnz_train) HIPC(hipMemcpyAsync(colids_train, w.d_colids, nnz_train * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (H) {
        HIPC(hipMemcpyAsync(held_u, w.d_hu, H * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipMemcpyAsync(held_v, w.d_hv, H * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (negs) {
        HIPC(hipMemcpyAsync(neg_u, w.d_nu, negs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipMemcpyAsync(neg_v, w.d_nv, negs * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    rowptr_train[n] = (uint32_t)nnz_train;
    if (info) {
        info->seconds = seconds;
        info->drawn = sums[11];
    }
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_edge_split(f2v_handle c, double frac, uint64_t seed, uint32_t ratio, uint32_t *rowptr_train, uint32_t *colids_train, uint64_t cap_train,
                   uint32_t *held_u, uint32_t *held_v, uint64_t cap_held, uint32_t *neg_u, uint32_t *neg_v, uint64_t cap_neg, uint64_t *train_nnz_out,
                   uint64_t *held_out, uint64_t *negatives_out, f2v_split_t *info) {
    return edge_split_impl(c, "f2v_edge_split", false, frac, seed, ratio, rowptr_train, colids_train, cap_train, held_u, held_v, cap_held, neg_u, neg_v, cap_neg,
                           train_nnz_out, held_out, negatives_out, info);
}

int f2v_edge_split_connected(f2v_handle c, double frac, uint64_t seed, uint32_t ratio, uint32_t *rowptr_train, uint32_t *colids_train, uint64_t cap_train,
                             uint32_t *held_u, uint32_t *held_v, uint64_t cap_held, uint32_t *neg_u, uint32_t *neg_v, uint64_t cap_neg,
                             uint64_t *train_nnz_out, uint64_t *held_out, uint64_t *negatives_out, f2v_split_t *info) {
    return edge_split_impl(c, "f2v_edge_split_connected", true, frac, seed, ratio, rowptr_train, colids_train, cap_train, held_u, held_v, cap_held, neg_u, neg_v,
                           cap_neg, train_nnz_out, held_out, negatives_out, info);
}

int f2v_pair_scores(f2v_handle c, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, int metric, float *scores_out, double *seconds_out) {
    if (!c) return fail(F2V_EINVAL, "f2v_pair_scores: null argument");
    if (metric != F2V_SIM_DOT && metric != F2V_SIM_L2 && metric != F2V_SIM_COSINE) return fail(F2V_EINVAL, "f2v_pair_scores: unknown metric %d", metric);
    if (seconds_out) *seconds_out = 0.0;
    if (m == 0 && c->have_x) return F2V_OK;
    if (m && (!u_ids || !v_ids || !scores_out)) return fail(F2V_EINVAL, "f2v_pair_scores: null argument");
    for (uint64_t i = 0; i < m; i++)
        if (u_ids[i] >= c->n || v_ids[i] >= c->n)
            return fail(F2V_EINVAL, "f2v_pair_scores: pair %llu = (%u, %u) names a vertex that is not one of the %u", (unsigned long long)i, u_ids[i], v_ids[i], c->n);
    F2VC(settled_enter(c, "f2v_pair_scores"));
    if (m == 0) return F2V_OK;

    f2v_ctx::Heldout &w = c->held;
    const char *what = "pair scores";
    const uint64_t chunk = std::min<uint64_t>(w.pairs_chunk, m);
    F2VC(w.d_pu.reserve(c, chunk, what));
    F2VC(w.d_pv.reserve(c, chunk, what));
    F2VC(w.d_ps.reserve(c, chunk, what));
    PairArgs a{};
    a.X = c->d_X[c->cur];
    a.u = w.d_pu;
    a.v = w.d_pv;
    a.out = w.d_ps;
    a.D = c->D;
    double seconds = 0.0;
    for (uint64_t i0 = 0; i0 < m; i0 += chunk) {
        const uint32_t cm = (uint32_t)std::min<uint64_t>(chunk, m - i0);
        a.m = cm;
        HIPC(hipMemcpyAsync(w.d_pu, u_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(w.d_pv, v_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        const dim3 grid(std::min((cm + 63u) / 64u, 65536u));
        F2VC(w.timer.start(c->stream));
        if (metric == F2V_SIM_DOT) hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_DOT>, grid, dim3(64), 0, c->stream, a);
        else if (metric == F2V_SIM_L2) hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_L2>, grid, dim3(64), 0, c->stream, a);
        else hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_COSINE>, grid, dim3(64), 0, c->stream, a);
        HIPC(hipGetLastError());
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(scores_out + i0, w.d_ps, (size_t)cm * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

int f2v_ranking(f2v_handle c, const double *scores, const uint8_t *y, uint64_t m, f2v_ranking_t *out) {
    if (!c || !out || (m && (!scores || !y))) return fail(F2V_EINVAL, "f2v_ranking: null argument");
    if (m >= (1ull << 31)) return fail(F2V_EINVAL, "f2v_ranking: m = %llu reaches 2^31", (unsigned long long)m);
    *out = f2v_ranking_t{};
    uint64_t P = 0;
    for (uint64_t i = 0; i < m; i++) {
        if (y[i] > 1) return fail(F2V_EINVAL, "f2v_ranking: y[%llu] = %u is neither 0 nor 1", (unsigned long long)i, (unsigned)y[i]);
        P += y[i];
    }
    const uint64_t N = m - P;
    out->positives = P;
    out->negatives = N;
    if (P == 0 || N == 0) return fail(F2V_EINVAL, "f2v_ranking: %llu ones and %llu zeros: both classes are needed", (unsigned long long)P, (unsigned long long)N);
    HIPC(hipSetDevice(c->device));

    f2v_ctx::Heldout &w = c->held;
    const char *what = "ranking";
    const uint32_t mm = (uint32_t)m, tiles = (mm + kLinkScanTile - 1) / kLinkScanTile, blocks = (mm + kRankBlock - 1) / kRankBlock;
    F2VC(w.d_scores.reserve(c, m, what));
    F2VC(w.d_keys[0].reserve(c, m, what));
    F2VC(w.d_keys[1].reserve(c, m, what));
    F2VC(w.d_labels[0].reserve(c, m, what));
    F2VC(w.d_labels[1].reserve(c, m, what));
    F2VC(w.d_cum.reserve(c, m, what));
    F2VC(w.d_terms.reserve(c, m, what));
    F2VC(w.d_blocks.reserve(c, (size_t)blocks + 1, what));  // the last word: the sum of the block sums
    F2VC(w.d_tile.reserve(c, tiles, what));
    F2VC(w.d_tallies.reserve(c, 3, what));
    size_t sort_bytes = 0;
    HIPC(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)w.d_keys[0], (unsigned long long *)w.d_keys[1], (uint8_t *)w.d_labels[0],
                                   (uint8_t *)w.d_labels[1], (size_t)mm, 0u, 64u, c->stream));
    F2VC(w.d_sort.reserve(c, sort_bytes, what));
    HIPC(hipMemcpyAsync(w.d_scores, scores, m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_labels[0], y, m * sizeof(uint8_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(w.d_tallies, 0, 3 * sizeof(unsigned long long), c->stream));
    RankArgs a{};
    a.scores = w.d_scores;
    a.keys = w.d_keys[0];
    a.cum = w.d_cum;
    a.tile = w.d_tile;
    a.terms = w.d_terms;
    a.blocks = w.d_blocks;
    a.ap_sum = w.d_blocks + blocks;
    a.tallies = w.d_tallies;
    a.negatives = N;
    a.m = mm;
    LinkArgs l{};  // link_scan_top_kernel reads its tile sums alone
    l.tile = w.d_tile;
    const dim3 grid(std::min((mm + 255u) / 256u, 65536u));
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(rank_key_kernel, grid, dim3(256), 0, c->stream, a);
    HIPC(rocprim::radix_sort_pairs((void *)(uint8_t *)w.d_sort, sort_bytes, (unsigned long long *)w.d_keys[0], (unsigned long long *)w.d_keys[1],
                                   (uint8_t *)w.d_labels[0], (uint8_t *)w.d_labels[1], (size_t)mm, 0u, 64u, c->stream));
    a.keys = w.d_keys[1];
    a.labels = w.d_labels[1];
    hipLaunchKernelGGL(rank_scan_tile_kernel, dim3(tiles), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(link_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, l, tiles);
    hipLaunchKernelGGL(rank_scan_apply_kernel, dim3(tiles), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(rank_group_kernel, grid, dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(rank_block_kernel, dim3((blocks + 63u) / 64u), dim3(64), 0, c->stream, a, blocks);
    hipLaunchKernelGGL(rank_total_kernel, dim3(1), dim3(64), 0, c->stream, a, blocks);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long tallies[3];
    double sum = 0.0, seconds = 0.0;
    HIPC(hipMemcpyAsync(tallies, w.d_tallies, sizeof tallies, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(&sum, w.d_blocks + blocks, sizeof sum, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    out->concordant = tallies[0];
    out->tied = tallies[1];
    out->groups = tallies[2];
    out->auc = (double)(2 * out->concordant + out->tied) / (2.0 * (double)P * (double)N);
    out->ap = sum / (double)P;
    out->seconds = seconds;
    return F2V_OK;
}

}  // extern "C"

// ---- neighbourhood scores of pairs (f2v_neighbourhood.hip.h; definition in include/f2v.h) -----------------------------------------
extern "C" {

int f2v_pair_neighbourhood(f2v_handle c, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, uint32_t kinds, double *scores_out, double *seconds_out) {
    if (!c) return fail(F2V_EINVAL, "f2v_pair_neighbourhood: null argument");
    if (kinds == 0 || (kinds & ~(uint32_t)F2V_NB_ALL)) return fail(F2V_EINVAL, "f2v_pair_neighbourhood: kinds = 0x%x names no score or an unknown one", kinds);
    if (seconds_out) *seconds_out = 0.0;
    if (m == 0) return F2V_OK;
    if (!u_ids || !v_ids || !scores_out) return fail(F2V_EINVAL, "f2v_pair_neighbourhood: null argument");
    for (uint64_t i = 0; i < m; i++)
        if (u_ids[i] >= c->n || v_ids[i] >= c->n)
            return fail(F2V_EINVAL, "f2v_pair_neighbourhood: pair %llu = (%u, %u) names a vertex that is not one of the %u", (unsigned long long)i, u_ids[i], v_ids[i], c->n);
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_pair_neighbourhood: the CSR's column ids are not ascending inside every row (needed to search a row)");
    HIPC(hipSetDevice(c->device));

    f2v_ctx::Neighbourhood &w = c->nb;
    const char *what = "neighbourhood scores";
    const uint32_t n = c->n, nk = (uint32_t)__builtin_popcount(kinds), rows = std::min((n + 3) / 4, 8192u);
    const bool search = (kinds & ~(uint32_t)F2V_NB_PREFERENTIAL) != 0, terms = (kinds & (F2V_NB_ADAMIC_ADAR | F2V_NB_RESOURCE)) != 0;
    const uint64_t chunk = std::min<uint64_t>(c->held.pairs_chunk, m);
    const uint32_t tiles = (uint32_t)((chunk + kLinkScanTile - 1) / kLinkScanTile);
    F2VC(w.d_deg.reserve(c, n, what));
    F2VC(w.d_u.reserve(c, chunk, what));
    F2VC(w.d_v.reserve(c, chunk, what));
    F2VC(w.d_out.reserve(c, chunk * nk, what));
    if (search) {
        F2VC(w.d_items_of.reserve(c, chunk, what));
        F2VC(w.d_zero.reserve(c, chunk, what));
        F2VC(w.d_offset.reserve(c, chunk, what));
        F2VC(w.d_tile.reserve(c, tiles, what));
        F2VC(w.d_sums.reserve(c, 1, what));
    }
    NbArgs a{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.deg = w.d_deg;
    a.u = w.d_u;
    a.v = w.d_v;
    a.items_of = w.d_items_of;
    a.zero = w.d_zero;
    a.offset = w.d_offset;
    a.sums = w.d_sums;
    a.out = w.d_out;
    a.n = n;
    a.kinds = kinds;
    a.spread = w.spread ? 1u : 0u;
    LinkArgs l{};  // the scan of f2v_linkpairs.hip.h over the chunk's pairs
    l.p = w.d_items_of;
    l.total = w.d_zero;
    l.offset = w.d_offset;
    l.tile = w.d_tile;
    double seconds = 0.0;
    w.last_items = 0;
    for (uint64_t i0 = 0; i0 < m; i0 += chunk) {
        const uint32_t cm = (uint32_t)std::min<uint64_t>(chunk, m - i0), ctiles = (cm + kLinkScanTile - 1) / kLinkScanTile;
        const dim3 per_pair(std::min((cm + 255u) / 256u, kNbThreadCap));
        a.m = l.n = cm;
        a.items = 0;
        HIPC(hipMemcpyAsync(w.d_u, u_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(w.d_v, v_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (search) HIPC(hipMemsetAsync(w.d_sums, 0, sizeof(unsigned long long), c->stream));
        F2VC(w.timer.start(c->stream));
        if (!w.degrees_built) hipLaunchKernelGGL(nb_degree_kernel, dim3(rows), dim3(256), 0, c->stream, a);
        if (search) {
            hipLaunchKernelGGL(nb_count_kernel, per_pair, dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL(link_scan_tile_kernel, dim3(ctiles), dim3(256), 0, c->stream, l);
            hipLaunchKernelGGL(link_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, l, ctiles);
            hipLaunchKernelGGL(link_scan_apply_kernel, dim3(ctiles), dim3(256), 0, c->stream, l);
            HIPC(hipGetLastError());
            F2VC(w.timer.stop(c->stream));
            unsigned long long items = 0;
            HIPC(hipMemcpyAsync(&items, w.d_sums, sizeof items, hipMemcpyDeviceToHost, c->stream));
            HIPC(hipStreamSynchronize(c->stream));
            F2VC(w.timer.seconds(&seconds));
            w.degrees_built = true;
            if (items) {
                F2VC(w.d_item.reserve(c, items, what));
                F2VC(w.d_piece_c.reserve(c, items, what));
                F2VC(w.d_piece_aa.reserve(c, items, what));
                F2VC(w.d_piece_ra.reserve(c, items, what));
            }
            a.items = items;
            a.item = w.d_item;
            a.piece_c = w.d_piece_c;
            a.piece_aa = w.d_piece_aa;
            a.piece_ra = w.d_piece_ra;
            w.last_items += items;
            const dim3 grid((unsigned)std::min<uint64_t>((items + cm + 3) / 4, kNbGridCap));
            F2VC(w.timer.start(c->stream));
            if (items) hipLaunchKernelGGL(nb_fill_kernel, per_pair, dim3(256), 0, c->stream, a);
            if (terms) hipLaunchKernelGGL(nb_pair_kernel<true>, grid, dim3(256), 0, c->stream, a);
            else hipLaunchKernelGGL(nb_pair_kernel<false>, grid, dim3(256), 0, c->stream, a);
            if (items) hipLaunchKernelGGL(nb_finish_kernel, per_pair, dim3(256), 0, c->stream, a, 0u);
        } else {
            hipLaunchKernelGGL(nb_finish_kernel, per_pair, dim3(256), 0, c->stream, a, 1u);  // the degree product alone: nothing is searched
        }
        HIPC(hipGetLastError());
        F2VC(w.timer.stop(c->stream));
        for (uint32_t k = 0; k < nk; k++)
            HIPC(hipMemcpyAsync(scores_out + (size_t)k * m + i0, w.d_out + (size_t)k * cm, (size_t)cm * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
        w.degrees_built = true;
    }
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

}  // extern "C"

// ---- ranks of pairs (f2v_pairranks.hip.h; definition in include/f2v.h) --------------------------------------------------------------
template <bool L2, int WQ, int MI, int NI>
int launch_prank_t(f2v_ctx *c, const PrankArgs &a, uint32_t qblocks, uint32_t splits) {
    const size_t lds = prank_lds_bytes(32u * WQ * MI, a.D);
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&prank_count_kernel<L2, WQ, MI, NI>), lds));
    hipLaunchKernelGGL((prank_count_kernel<L2, WQ, MI, NI>), dim3(qblocks, splits), dim3(kNnThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

extern "C" {

int f2v_pair_ranks(f2v_handle c, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, int metric, uint32_t flags, uint32_t *greater_out,
                   uint32_t *equal_out, const uint32_t *ks, uint32_t nk, uint64_t *hits_out, f2v_pair_ranks_t *info) {
    const char *who = "f2v_pair_ranks";
    if (!c || (m && (!u_ids || !v_ids || !greater_out || !equal_out)) || (nk && (!ks || !hits_out))) return fail(F2V_EINVAL, "%s: null argument", who);
    if (nk > F2V_RANKS_MAX_KS) return fail(F2V_EINVAL, "%s: nk = %u is above %d", who, nk, F2V_RANKS_MAX_KS);
    for (uint32_t j = 0; j < nk; j++)
        if (ks[j] == 0) return fail(F2V_EINVAL, "%s: ks[%u] is 0", who, j);
    for (uint64_t i = 0; i < m; i++)
        if (u_ids[i] >= c->n || v_ids[i] >= c->n)
            return fail(F2V_EINVAL, "%s: pair %llu = (%u, %u) names a vertex that is not one of the %u", who, (unsigned long long)i, u_ids[i], v_ids[i], c->n);
    if (info) *info = f2v_pair_ranks_t{};
    for (uint32_t j = 0; j < nk; j++) hits_out[j] = 0;
    const bool by_row = (flags & F2V_NEAREST_EXCLUDE_NEIGHBOURS) != 0;
    const int rc = nearest_enter(c, who, m ? 1u : 0u, 1, metric, flags, by_row);  // (no k here: 1 passes its range check)
    if (rc) return rc < 0 ? rc : F2V_OK;

    f2v_ctx::Ranks &w = c->pr;
    const char *what = "pair ranks";
    const uint32_t n = c->n, D = c->D, tiles = (n + kNnTile - 1) / kNnTile;
    const bool cosine = metric == F2V_SIM_COSINE;
    const float *X = c->d_X[c->cur];
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(w.chunk, m);
    F2VC(w.d_u.reserve(c, chunk, what));
    F2VC(w.d_v.reserve(c, chunk, what));
    F2VC(w.d_t.reserve(c, chunk, what));
    F2VC(w.d_greater.reserve(c, chunk, what));
    F2VC(w.d_equal.reserve(c, chunk, what));
    F2VC(w.d_Q.reserve(c, (size_t)chunk * D, what));
    F2VC(w.d_excluded.reserve(c, 1, what));
    if (cosine) F2VC(w.d_rc.reserve(c, n, what));
    PrankArgs a{};
    a.X = X;
    a.Q = w.d_Q;
    a.rc = cosine ? (const float *)w.d_rc : nullptr;
    a.t = w.d_t;
    a.u = w.d_u;
    a.v = w.d_v;
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.greater = w.d_greater;
    a.equal = w.d_equal;
    a.excluded = w.d_excluded;
    a.n = n;
    a.D = D;
    a.flags = flags;
    PairArgs t{};
    t.X = X;
    t.u = w.d_u;
    t.v = w.d_v;
    t.out = w.d_t;
    t.D = D;
    double seconds[3] = {0.0, 0.0, 0.0};
    uint64_t excluded = 0;
    std::vector<PrankItem> items;
    for (uint64_t i0 = 0; i0 < m; i0 += chunk) {
        const uint32_t cm = (uint32_t)std::min<uint64_t>(chunk, m - i0);
        // the correction's work items: the pair itself, then -- under EXCLUDE_NEIGHBOURS -- the pieces of row u
        items.clear();
        for (uint32_t i = 0; i < cm; i++) {
            items.push_back({i, kPrankPairItem});
            const uint32_t u = u_ids[i0 + i], pieces = by_row ? (c->rowptr[u + 1] - c->rowptr[u] + kPrankPiece - 1) / kPrankPiece : 0u;
            for (uint32_t p = 0; p < pieces; p++) items.push_back({i, p});
        }
        if (items.size() > 0x7FFFFFFFull) return fail(F2V_EINVAL, "%s: a chunk of %u pairs has %zu work items: lower \"ranks_chunk\"", who, cm, items.size());
        F2VC(w.d_item.reserve(c, items.size(), what));
        const uint32_t qb = D <= 128 && cm > 32 ? 128u : 32u, qblocks = (cm + qb - 1) / qb;
        uint32_t splits = w.splits ? w.splits : std::min((1024u + qblocks - 1) / qblocks, 256u);  // workgroups for every CU a few times over
        splits = std::min(splits, tiles);
        const uint32_t tps = (tiles + splits - 1) / splits;
        splits = (tiles + tps - 1) / tps;
        a.nq = t.m = cm;
        a.tiles_per_split = tps;
        a.item = w.d_item;
        a.items = (uint32_t)items.size();
        HIPC(hipMemcpyAsync(w.d_u, u_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(w.d_v, v_ids + i0, (size_t)cm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(w.d_item, items.data(), items.size() * sizeof(PrankItem), hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemsetAsync(w.d_greater, 0, (size_t)cm * sizeof(uint32_t), c->stream));
        HIPC(hipMemsetAsync(w.d_equal, 0, (size_t)cm * sizeof(uint32_t), c->stream));
        HIPC(hipMemsetAsync(w.d_excluded, 0, sizeof(unsigned long long), c->stream));
        F2VC(w.timer[0].start(c->stream));
        hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)cm * D + 255) / 256, 4096)), dim3(256), 0, c->stream, X, (const uint32_t *)w.d_u, cm, D, w.d_Q);
        if (cosine && i0 == 0) hipLaunchKernelGGL(nearest_rnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, X, n, D, w.d_rc);
        const dim3 tgrid((cm + 63u) / 64u);  // (a chunk has at most 65536 pairs)
        if (metric == F2V_SIM_DOT) hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_DOT>, tgrid, dim3(64), 0, c->stream, t);
        else if (metric == F2V_SIM_L2) hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_L2>, tgrid, dim3(64), 0, c->stream, t);
        else hipLaunchKernelGGL(pair_score_kernel<F2V_SIM_COSINE>, tgrid, dim3(64), 0, c->stream, t);
        HIPC(hipGetLastError());
        F2VC(w.timer[0].stop(c->stream));
        F2VC(w.timer[1].start(c->stream));
        if (metric == F2V_SIM_L2) F2VC((qb == 128 ? launch_prank_t<true, 2, 2, 2>(c, a, qblocks, splits) : launch_prank_t<true, 1, 1, 1>(c, a, qblocks, splits)));
        else F2VC((qb == 128 ? launch_prank_t<false, 2, 2, 2>(c, a, qblocks, splits) : launch_prank_t<false, 1, 1, 1>(c, a, qblocks, splits)));
        F2VC(w.timer[1].stop(c->stream));
        F2VC(w.timer[2].start(c->stream));
        const dim3 cgrid(a.items);  // a workgroup of one wavefront per item (below 2^31: checked above)
        if (metric == F2V_SIM_DOT) hipLaunchKernelGGL(prank_correct_kernel<F2V_SIM_DOT>, cgrid, dim3(64), 0, c->stream, a);
        else if (metric == F2V_SIM_L2) hipLaunchKernelGGL(prank_correct_kernel<F2V_SIM_L2>, cgrid, dim3(64), 0, c->stream, a);
        else hipLaunchKernelGGL(prank_correct_kernel<F2V_SIM_COSINE>, cgrid, dim3(64), 0, c->stream, a);
        HIPC(hipGetLastError());
        F2VC(w.timer[2].stop(c->stream));
        unsigned long long ex = 0;
        HIPC(hipMemcpyAsync(greater_out + i0, w.d_greater, (size_t)cm * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipMemcpyAsync(equal_out + i0, w.d_equal, (size_t)cm * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipMemcpyAsync(&ex, w.d_excluded, sizeof ex, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 3; k++) F2VC(w.timer[k].seconds(&seconds[k]));
        excluded += ex;
    }
    F2VC(check_kernel_err(c, "pair ranks"));
    w.base_seconds = seconds[1];
    w.correct_seconds = seconds[2];

    // the summary, from the integers: rank2 = 2 + 2 greater + equal, twice the mid-rank
    uint64_t rank2_sum = 0, tied = 0;
    double mrr_sum = 0.0;
    for (uint64_t b0 = 0; b0 < m; b0 += 1024) {  // blocks of 1024 pairs, each summed from +0 in input order, then added in ascending order
        double block = 0.0;
        for (uint64_t i = b0; i < std::min(m, b0 + 1024); i++) {
            const uint64_t rank2 = 2 + 2 * (uint64_t)greater_out[i] + equal_out[i];
            rank2_sum += rank2;
            tied += equal_out[i] ? 1u : 0u;
            block += 2.0 / (double)rank2;
            for (uint32_t j = 0; j < nk; j++) hits_out[j] += rank2 <= 2 * (uint64_t)ks[j] ? 1u : 0u;
        }
        mrr_sum += block;
    }
    if (info) {
        info->seconds = seconds[0] + seconds[1] + seconds[2];
        info->pairs = m;
        info->rank2_sum = rank2_sum;
        info->mean_rank = (double)rank2_sum / (2.0 * (double)m);
        info->mrr = mrr_sum / (double)m;
        info->candidates = m * (uint64_t)(n - 1) - excluded;
        info->tied_pairs = tied;
    }
    return F2V_OK;
}

}  // extern "C"

// ---- communities and the agreement of two labellings (f2v_louvain.hip.h; definition in include/f2v.h) ---------------------------
namespace {

constexpr const char *kLouvainWhat = "communities";

inline dim3 louvain_grid(uint64_t threads) { return dim3((unsigned)std::max<uint64_t>(1, (threads + 255) / 256)); }

// Is every nonzero (u, v), u != v, matched by (v, u)?  Checked once per handle, on the device (rows ascending: rows_ascending first).
int rows_symmetric(f2v_ctx *c, bool *yes) {
    f2v_ctx::Louvain &w = c->lv;
    if (w.rows_symmetric < 0) {
        F2VC(w.d_flag.reserve(c, 1, kLouvainWhat));
        HIPC(hipMemsetAsync(w.d_flag, 0, sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(louvain_symmetry_kernel, dim3(std::max(1u, std::min((c->n + 15) / 16, 16384u))), dim3(256), 0, c->stream, c->d_rowptr, c->d_colids, c->n,
                           (uint32_t *)w.d_flag);
        HIPC(hipGetLastError());
        uint32_t bad = 0;
        HIPC(hipMemcpyAsync(&bad, w.d_flag, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        w.rows_symmetric = bad ? 0 : 1;
    }
    *yes = w.rows_symmetric == 1;
    return F2V_OK;
}

// exclusive prefix sums of x[0 .. count) in place, the total to x[count]
int louvain_scan(f2v_ctx *c, uint32_t *x, uint64_t count) {
    f2v_ctx::Louvain &w = c->lv;
    const uint32_t tiles = (uint32_t)std::max<uint64_t>(1, (count + kLouvainScanTile - 1) / kLouvainScanTile);
    F2VC(w.d_tile.reserve(c, tiles, kLouvainWhat));
    hipLaunchKernelGGL(louvain_scan_tile_kernel, dim3(tiles), dim3(256), 0, c->stream, (const uint32_t *)x, count, (uint32_t *)w.d_tile);
    hipLaunchKernelGGL(louvain_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, (uint32_t *)w.d_tile, tiles, x + count);
    hipLaunchKernelGGL(louvain_scan_apply_kernel, dim3(tiles), dim3(256), 0, c->stream, x, count, (const uint32_t *)w.d_tile);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// The lists of `count` units by (class, form): counted, read back (32 words), filled.  cnt[0..23]: units per list, a.start: their places.
int louvain_place(f2v_ctx *c, LouvainArgs &a, uint32_t count, bool agg, unsigned long long cnt[32]) {
    f2v_ctx::Louvain &w = c->lv;
    HIPC(hipMemsetAsync(w.d_bins, 0, 64 * sizeof(unsigned long long), c->stream));
    a.count = count;
    a.agg = agg ? 1u : 0u;
    a.bins = w.d_bins;
    hipLaunchKernelGGL(louvain_bin_kernel<false>, louvain_grid(count), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(cnt, w.d_bins, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    uint64_t units = 0, words = 0;
    for (uint32_t b = 0; b < kLouvainBins; b++) {
        a.start[b] = (uint32_t)units;
        units += cnt[b];
    }
    for (uint32_t p = 0; p < F2V_LOUVAIN_PHASES; p++) words = std::max<uint64_t>(words, cnt[kLouvainBins + p]);  // sub-rounds follow one another: one table space
    F2VC(w.d_units.reserve(c, units, kLouvainWhat));
    F2VC(w.d_table_at.reserve(c, units, kLouvainWhat));
    F2VC(w.d_table.reserve(c, words, kLouvainWhat));
    a.units = w.d_units;
    a.table_at = w.d_table_at;
    a.table = w.d_table;
    if (units) hipLaunchKernelGGL(louvain_bin_kernel<true>, louvain_grid(count), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// the three forms of class `cls`
template <bool AGG>
int louvain_gather(f2v_ctx *c, LouvainArgs a, const unsigned long long *cnt, uint32_t cls) {
    f2v_ctx::Louvain &w = c->lv;
    for (uint32_t form = 0; form < 3; form++) {
        const uint32_t bin = cls * 3 + form;
        if (!cnt[bin]) continue;
        a.units = w.d_units + a.start[bin];
        a.table_at = w.d_table_at + a.start[bin];
        a.count = (uint32_t)cnt[bin];
        if (form == 0) {
            a.slots = louvain_slots(a.short_max);
            const size_t lds = (kLouvainHeader + 32 * (size_t)a.slots) * sizeof(uint32_t);
            F2VC(allow_lds(c, reinterpret_cast<const void *>(&louvain_gather_kernel<0, AGG>), lds));
            hipLaunchKernelGGL((louvain_gather_kernel<0, AGG>), dim3(std::min((a.count + 15) / 16, 16384u)), dim3(256), lds, c->stream, a);
        } else if (form == 1) {
            const size_t lds = (kLouvainHeader + 2 * (size_t)a.lds_slots) * sizeof(uint32_t);
            F2VC(allow_lds(c, reinterpret_cast<const void *>(&louvain_gather_kernel<1, AGG>), lds));
            hipLaunchKernelGGL((louvain_gather_kernel<1, AGG>), dim3(std::min(a.count, 65536u)), dim3(256), lds, c->stream, a);
        } else {
            hipLaunchKernelGGL((louvain_gather_kernel<2, AGG>), dim3(std::min(a.count, 65536u)), dim3(kLouvainWideThreads), kLouvainHeader * sizeof(uint32_t), c->stream, a);
        }
    }
    HIPC(hipGetLastError());
    return F2V_OK;
}

// Qnum of the labelling c: the two sums, then in2 * 2m - sum tot^2
int louvain_qnum(f2v_ctx *c, const LouvainArgs &a, const unsigned long long *cnt, unsigned long long sums[3]) {
    hipLaunchKernelGGL(louvain_qnum_kernel, dim3(std::max(1u, std::min((a.N + 15) / 16, 16384u))), dim3(256), 0, c->stream, a);
    for (uint32_t p = 0; p < F2V_LOUVAIN_PHASES; p++) {  // the rows it leaves out: the third list of every class
        if (!cnt[3 * p + 2]) continue;
        LouvainArgs wide = a;
        wide.units = c->lv.d_units + a.start[3 * p + 2];
        wide.count = (uint32_t)cnt[3 * p + 2];
        hipLaunchKernelGGL(louvain_qnum_wide_kernel, dim3(std::min(wide.count, 65536u)), dim3(256), 0, c->stream, wide);
    }
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(sums, a.sums, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_louvain(f2v_handle c, uint64_t seed, uint32_t max_levels, uint32_t max_sweeps, uint32_t *labels_out, uint32_t *level_labels_out,
                f2v_louvain_level_t *levels_out, f2v_louvain_t *info_out) {
    if (!c || !labels_out || !info_out) return fail(F2V_EINVAL, "f2v_louvain: null argument");
    if (max_levels == 0 || max_sweeps == 0) return fail(F2V_EINVAL, "f2v_louvain: max_levels and max_sweeps must be at least 1");
    HIPC(hipSetDevice(c->device));
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_louvain: the CSR's column ids are not ascending inside every row (needed to search a row)");
    bool symmetric = false;
    F2VC(rows_symmetric(c, &symmetric));
    if (!symmetric) return fail(F2V_EINVAL, "f2v_louvain: the CSR is not structurally symmetric: a nonzero (u, v) without (v, u)");
    *info_out = f2v_louvain_t{};
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;

    f2v_ctx::Louvain &w = c->lv;
    const char *what = kLouvainWhat;
    F2VC(w.d_k[0].reserve(c, n, what));
    F2VC(w.d_loop[0].reserve(c, n, what));
    F2VC(w.d_c.reserve(c, n, what));
    F2VC(w.d_next.reserve(c, n, what));
    F2VC(w.d_tot.reserve(c, n, what));
    F2VC(w.d_size.reserve(c, n, what));
    F2VC(w.d_kept.reserve(c, n, what));
    F2VC(w.d_newid.reserve(c, (size_t)n + 1, what));
    F2VC(w.d_ccount.reserve(c, (size_t)n + 1, what));
    F2VC(w.d_members.reserve(c, n, what));
    F2VC(w.d_vlabel.reserve(c, n, what));
    F2VC(w.d_sums.reserve(c, 8, what));
    F2VC(w.d_bins.reserve(c, 64, what));
    HIPC(hipMemsetAsync(w.d_sums, 0, 8 * sizeof(unsigned long long), c->stream));
    F2VC(w.timer.start(c->stream));
    const dim3 rows16(std::max(1u, std::min((n + 15) / 16, 16384u)));
    hipLaunchKernelGGL(louvain_degree_kernel, rows16, dim3(256), 0, c->stream, c->d_rowptr, c->d_colids, n, (uint32_t *)w.d_k[0], (uint32_t *)w.d_loop[0],
                       (unsigned long long *)w.d_sums);
    hipLaunchKernelGGL(louvain_iota_kernel, louvain_grid(n), dim3(256), 0, c->stream, (uint32_t *)w.d_vlabel, n);
    HIPC(hipGetLastError());
    unsigned long long two_m = 0;
    HIPC(hipMemcpyAsync(&two_m, w.d_sums + 3, sizeof two_m, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (two_m >= (1ull << 31)) {
        F2VC(w.timer.stop(c->stream));
        return fail(F2V_EINVAL, "f2v_louvain: the degrees sum to %llu, not below 2^31", two_m);
    }

    LouvainArgs a{};
    a.rowbeg = c->d_rowptr;
    a.rowend = c->d_rowptr + 1;
    a.cols = c->d_colids;
    a.wts = nullptr;
    a.dedupe = 1;
    a.N = a.n = n;
    a.two_m = (uint32_t)two_m;
    a.c = w.d_c;
    a.next = w.d_next;
    a.tot = w.d_tot;
    a.size = w.d_size;
    a.kept = w.d_kept;
    a.vlabel = w.d_vlabel;
    a.sums = w.d_sums;
    a.short_max = w.short_max;
    a.lds_slots = w.lds_slots;
    uint32_t levels = 0, communities = n;
    for (uint32_t level = 0; level < max_levels; level++) {
        const uint32_t set = level & 1u, out = set ^ 1u, N = a.N;
        a.k = w.d_k[set];
        a.loop = w.d_loop[set];
        a.key = a.c;
        a.level_mix = mix64_host(seed + level);
        hipLaunchKernelGGL(louvain_init_kernel, louvain_grid(N), dim3(256), 0, c->stream, a);
        unsigned long long cnt[32], sums[3];
        F2VC(louvain_place(c, a, N, false, cnt));
        HIPC(hipMemsetAsync(w.d_sums, 0, 3 * sizeof(unsigned long long), c->stream));
        F2VC(louvain_qnum(c, a, cnt, sums));
        const int64_t start = (int64_t)(sums[1] * two_m) - (int64_t)sums[2];
        int64_t best = start;
        uint32_t sweeps = 0;
        uint64_t moves = 0;
        while (sweeps < max_sweeps) {
            HIPC(hipMemsetAsync(w.d_sums, 0, 3 * sizeof(unsigned long long), c->stream));
            for (uint32_t p = 0; p < F2V_LOUVAIN_PHASES; p++) {
                if (cnt[3 * p] + cnt[3 * p + 1] + cnt[3 * p + 2] == 0) continue;
                F2VC(louvain_gather<false>(c, a, cnt, p));
                hipLaunchKernelGGL(louvain_apply_kernel, louvain_grid(N), dim3(256), 0, c->stream, a);
            }
            F2VC(louvain_qnum(c, a, cnt, sums));
            sweeps++;
            moves += sums[0];
            const int64_t q = (int64_t)(sums[1] * two_m) - (int64_t)sums[2];
            if (q <= best) break;
            best = q;
            HIPC(hipMemcpyAsync(w.d_kept, w.d_c, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        }

        // aggregation: the kept communities renumbered in ascending id, the members grouped, the coarse rows gathered
        uint32_t K = N;
        if (best != start) {
            HIPC(hipMemsetAsync(w.d_newid, 0, ((size_t)N + 1) * sizeof(uint32_t), c->stream));
            a.newid = w.d_newid;
            hipLaunchKernelGGL(louvain_flag_kernel, louvain_grid(N), dim3(256), 0, c->stream, a);
            F2VC(louvain_scan(c, w.d_newid, N));
            HIPC(hipMemcpyAsync(&K, w.d_newid + N, sizeof K, hipMemcpyDeviceToHost, c->stream));
            HIPC(hipStreamSynchronize(c->stream));
            F2VC(w.d_rowbeg[out].reserve(c, (size_t)K + 1, what));
            F2VC(w.d_rowend[out].reserve(c, K, what));
            F2VC(w.d_k[out].reserve(c, K, what));
            F2VC(w.d_loop[out].reserve(c, K, what));
            HIPC(hipMemsetAsync(w.d_rowbeg[out], 0, ((size_t)K + 1) * sizeof(uint32_t), c->stream));
            HIPC(hipMemsetAsync(w.d_k[out], 0, (size_t)K * sizeof(uint32_t), c->stream));
            HIPC(hipMemsetAsync(w.d_loop[out], 0, (size_t)K * sizeof(uint32_t), c->stream));
            HIPC(hipMemsetAsync(w.d_ccount, 0, ((size_t)K + 1) * sizeof(uint32_t), c->stream));
            HIPC(hipMemsetAsync(w.d_size, 0, (size_t)K * sizeof(uint32_t), c->stream));  // (the cursors of louvain_member_fill_kernel)
            a.orowbeg = w.d_rowbeg[out];
            a.orowend = w.d_rowend[out];
            a.ok = w.d_k[out];
            a.oloop = w.d_loop[out];
            a.ccount = w.d_ccount;
            a.mstart = w.d_ccount;
            a.members = w.d_members;
            hipLaunchKernelGGL(louvain_member_count_kernel, louvain_grid(N), dim3(256), 0, c->stream, a);
            F2VC(louvain_scan(c, w.d_ccount, K));
            F2VC(louvain_scan(c, w.d_rowbeg[out], K));
            uint32_t nnz_out = 0;
            HIPC(hipMemcpyAsync(&nnz_out, w.d_rowbeg[out] + K, sizeof nnz_out, hipMemcpyDeviceToHost, c->stream));
            HIPC(hipStreamSynchronize(c->stream));
            F2VC(w.d_cols[out].reserve(c, nnz_out, what));
            F2VC(w.d_wts[out].reserve(c, nnz_out, what));
            a.ocols = w.d_cols[out];
            a.owts = w.d_wts[out];
            hipLaunchKernelGGL(louvain_member_fill_kernel, louvain_grid(N), dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL(louvain_relabel_kernel, louvain_grid(n), dim3(256), 0, c->stream, a);
            a.K = K;
            F2VC(louvain_place(c, a, K, true, cnt));
            a.key = a.next;
            F2VC(louvain_gather<true>(c, a, cnt, 0));
            a.rowbeg = w.d_rowbeg[out];
            a.rowend = w.d_rowend[out];
            a.cols = w.d_cols[out];
            a.wts = w.d_wts[out];
            a.dedupe = 0;
            a.N = K;
        }
        HIPC(hipGetLastError());
        if (level_labels_out)
            HIPC(hipMemcpyAsync(level_labels_out + (size_t)level * n, w.d_vlabel, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (levels_out) levels_out[level] = f2v_louvain_level_t{N, K, sweeps, 0u, moves, best};
        levels = level + 1;
        communities = K;
        if (best == start) break;  // an identity level: nothing left to merge
    }
    F2VC(w.timer.stop(c->stream));
    HIPC(hipMemcpyAsync(labels_out, w.d_vlabel, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&info_out->seconds));
    info_out->communities = communities;
    info_out->levels = levels;
    info_out->edges = two_m / 2;
    uint64_t edges = 0;
    F2VC(f2v_modularity(c, labels_out, communities, &info_out->modularity, &edges, nullptr, nullptr));
    return F2V_OK;
}

int f2v_partition_agreement(f2v_handle c, const uint32_t *la, uint32_t ka, const uint32_t *lb, uint32_t kb, f2v_agreement_t *out) {
    if (!c || !la || !lb || !out) return fail(F2V_EINVAL, "f2v_partition_agreement: null argument");
    if (ka == 0 || kb == 0) return fail(F2V_EINVAL, "f2v_partition_agreement: ka and kb must be at least 1");
    const uint64_t cells = (uint64_t)ka * kb;
    if (cells > F2V_AGREEMENT_MAX_CELLS) return fail(F2V_EINVAL, "f2v_partition_agreement: ka * kb = %llu cells are more than %u", (unsigned long long)cells, F2V_AGREEMENT_MAX_CELLS);
    const uint32_t n = c->n;
    uint64_t both = 0;
    for (uint32_t v = 0; v < n; v++) {
        if (la[v] != F2V_LABEL_NONE && la[v] >= ka) return fail(F2V_EINVAL, "f2v_partition_agreement: a[%u] = %u is not below ka = %u", v, la[v], ka);
        if (lb[v] != F2V_LABEL_NONE && lb[v] >= kb) return fail(F2V_EINVAL, "f2v_partition_agreement: b[%u] = %u is not below kb = %u", v, lb[v], kb);
        both += la[v] != F2V_LABEL_NONE && lb[v] != F2V_LABEL_NONE;
    }
    if (both < 2) return fail(F2V_EINVAL, "f2v_partition_agreement: %llu vertices are labelled in both, fewer than 2", (unsigned long long)both);
    HIPC(hipSetDevice(c->device));
    f2v_ctx::Louvain &w = c->lv;
    const char *what = kLouvainWhat;
    const uint64_t words = cells + ka + kb;
    const uint64_t pc = (cells + kAgreePiece - 1) / kAgreePiece, pa = ((uint64_t)ka + kAgreePiece - 1) / kAgreePiece, pb = ((uint64_t)kb + kAgreePiece - 1) / kAgreePiece;
    const uint64_t pieces = pc + pa + pb;
    F2VC(w.d_a.reserve(c, n, what));
    F2VC(w.d_b.reserve(c, n, what));
    F2VC(w.d_cells.reserve(c, words, what));
    F2VC(w.d_sums.reserve(c, 8, what));
    F2VC(w.d_pieces.reserve(c, pieces + 1, what));
    HIPC(hipMemcpyAsync(w.d_a, la, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_b, lb, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(w.d_cells, 0, words * sizeof(uint32_t), c->stream));
    HIPC(hipMemsetAsync(w.d_sums, 0, 8 * sizeof(unsigned long long), c->stream));
    AgreeArgs g{};
    g.a = w.d_a;
    g.b = w.d_b;
    g.cells = w.d_cells;
    g.sums = w.d_sums;
    g.pieces = w.d_pieces;
    g.cells_count = cells;
    g.n = n;
    g.ka = ka;
    g.kb = kb;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(agree_count_kernel, louvain_grid(n), dim3(256), 0, c->stream, g);
    hipLaunchKernelGGL(agree_piece_kernel, louvain_grid(pc), dim3(256), 0, c->stream, g, 0u, (uint64_t)0, cells, (uint64_t)0);
    hipLaunchKernelGGL(agree_piece_kernel, louvain_grid(pa), dim3(256), 0, c->stream, g, 1u, cells, (uint64_t)ka, pc);
    hipLaunchKernelGGL(agree_piece_kernel, louvain_grid(pb), dim3(256), 0, c->stream, g, 2u, cells + ka, (uint64_t)kb, pc + pa);
    hipLaunchKernelGGL(agree_log_kernel, dim3(1), dim3(1), 0, c->stream, g, pieces);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long sums[8];
    std::vector<double> piece(pieces + 1);
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(piece.data(), w.d_pieces, (pieces + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    *out = f2v_agreement_t{};
    F2VC(w.timer.seconds(&out->seconds));
    auto chain = [&](uint64_t lo, uint64_t cnt) {  // the piece sums, added in order from +0
        double s = 0.0;
        for (uint64_t p = 0; p < cnt; p++) s = s + piece[lo + p];
        return s;
    };
    const double S_ab = chain(0, pc), S_a = chain(pc, pa), S_b = chain(pc + pa, pb), logN = piece[pieces];
    const uint64_t N = sums[0];
    const double Nf = (double)N;
    out->n = N;
    out->sum_comb = sums[1];
    out->sum_a = sums[2];
    out->sum_b = sums[3];
    out->total = N * (N - 1) / 2;
    out->rows = (uint32_t)sums[5];
    out->cols = (uint32_t)sums[6];
    // a side with one non-empty class has no entropy and shares no information: decided on the integers, not on a rounded difference
    out->entropy_a = out->rows == 1 ? 0.0 : logN - S_a / Nf;
    out->entropy_b = out->cols == 1 ? 0.0 : logN - S_b / Nf;
    const double mi = (out->rows == 1 || out->cols == 1) ? 0.0 : (S_ab - S_a - S_b) / Nf + logN;
    out->mi = mi > 0.0 ? mi : 0.0;
    out->nmi = (out->entropy_a == 0.0 && out->entropy_b == 0.0) ? 1.0 : out->mi / (0.5 * (out->entropy_a + out->entropy_b));
    const double sc = (double)out->sum_comb, sa = (double)out->sum_a, sb = (double)out->sum_b, tt = (double)out->total;
    const double den = 0.5 * (sa + sb) - sa * sb / tt;
    out->ari = den == 0.0 ? 1.0 : (sc - sa * sb / tt) / den;
    return F2V_OK;
}

}  // extern "C"

// ---- components, spanning forests and subgraphs (f2v_components.hip.h; definition in include/f2v.h) ------------------------------
namespace {

constexpr const char *kCcWhat = "components";

inline dim3 cc_grid(uint64_t threads) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((threads + 255) / 256, 16384))); }

// What the graph calls share: the graph's arrays, the pieces of the long rows (built once per handle, from the host's rowptr), the
// two label arrays and the words the kernels report through
int cc_prepare(f2v_ctx *c, CcArgs &a) {
    f2v_ctx::Components &w = c->cc;
    const uint32_t n = c->n;
    if (!w.items_built) {
        std::vector<CcItem> items;
        for (uint32_t u = 0; u < n; u++) {
            const uint32_t lo = c->rowptr[u], hi = c->rowptr[u + 1];
            if (hi - lo <= kCcPiece) continue;
            for (uint32_t q = lo; q < hi; q += std::min(kCcPiece, hi - q)) items.push_back(CcItem{u, q, q + std::min(kCcPiece, hi - q)});
        }
        if (items.size() > 0xFFFFFFFFull) return fail(F2V_EINVAL, "components: too many row pieces");
        F2VC(w.d_items.reserve(c, items.size(), kCcWhat));
        if (!items.empty()) {
            HIPC(hipMemcpyAsync(w.d_items, items.data(), items.size() * sizeof(CcItem), hipMemcpyHostToDevice, c->stream));
            HIPC(hipStreamSynchronize(c->stream));  // (the vector goes out of scope)
        }
        w.nitems = (uint32_t)items.size();
        w.items_built = true;
    }
    F2VC(w.d_L.reserve(c, n, kCcWhat));
    F2VC(w.d_P.reserve(c, n, kCcWhat));
    F2VC(w.d_sums.reserve(c, 8, kCcWhat));
    a = CcArgs{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.items = w.d_items;
    a.n = n;
    a.nitems = w.nitems;
    a.L = w.d_L;
    a.P = w.d_P;
    a.sums = w.d_sums;
    HIPC(hipMemsetAsync(w.d_sums, 0, 8 * sizeof(unsigned long long), c->stream));
    return F2V_OK;
}

inline dim3 cc_piece_grid(const CcArgs &a) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)a.n + a.nitems + 3) / 4, 16384))); }

// P flattened (every vertex names its root), then L = P.  *flag0: what sums[0] held (a hook happened / a pair was found); it is cleared.
int cc_flatten(f2v_ctx *c, const CcArgs &a, bool *flag0) {
    f2v_ctx::Components &w = c->cc;
    for (;;) {
        hipLaunchKernelGGL(cc_jump_kernel, cc_grid(a.n), dim3(256), 0, c->stream, a);
        HIPC(hipGetLastError());
        unsigned long long flags[2];
        HIPC(hipMemcpyAsync(flags, w.d_sums, sizeof flags, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipMemsetAsync(w.d_sums, 0, sizeof flags, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        if (flags[0]) *flag0 = true;
        if (!flags[1]) break;
    }
    HIPC(hipMemcpyAsync(w.d_L, w.d_P, (size_t)a.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return F2V_OK;
}

struct ForestRun {
    uint64_t edges = 0, forest_edges = 0;
    uint32_t rounds = 0;
    double seconds = 0.0;
};

// Boruvka over the order of (seed, "forest_key_bits", greatest): the sorted packed pairs end in c->cc.d_forest[1]
int forest_run(f2v_ctx *c, uint64_t seed, uint32_t greatest, ForestRun &out) {
    f2v_ctx::Components &w = c->cc;
    const uint32_t n = c->n;
    bool symmetric = false;
    F2VC(rows_symmetric(c, &symmetric));
    CcArgs a;
    F2VC(cc_prepare(c, a));
    F2VC(w.d_best1.reserve(c, n, kCcWhat));
    F2VC(w.d_best2.reserve(c, n, kCcWhat));
    F2VC(w.d_forest[0].reserve(c, n, kCcWhat));
    F2VC(w.d_forest[1].reserve(c, n, kCcWhat));
    a.best1 = w.d_best1;
    a.best2 = w.d_best2;
    a.forest = w.d_forest[0];
    a.se = mix64_host(mix64_host(seed) ^ 0x65646765ull);
    a.shift = 64u - w.key_bits;
    a.greatest = greatest;
    a.both = symmetric ? 0u : 1u;
    w.round_seconds.clear();
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(cc_iota_kernel, cc_grid(n), dim3(256), 0, c->stream, (uint32_t *)w.d_L, (uint32_t *)w.d_P, n);
    hipLaunchKernelGGL(cc_edges_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    for (;;) {
        const auto t0 = std::chrono::steady_clock::now();
        HIPC(hipMemsetAsync(w.d_best1, 0, (size_t)n * sizeof(unsigned long long), c->stream));
        HIPC(hipMemsetAsync(w.d_best2, 0, (size_t)n * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(forest_key_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL(forest_pair_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL(forest_hook_kernel, cc_grid(n), dim3(256), 0, c->stream, a);
        bool found = false;
        F2VC(cc_flatten(c, a, &found));
        out.rounds++;
        w.round_seconds.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (!found) break;
    }
    unsigned long long sums[8];
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    out.edges = sums[2];
    out.forest_edges = sums[6];
    if (out.forest_edges >= n) return fail(F2V_ESTATE, "spanning forest: %llu pairs on %u vertices", (unsigned long long)out.forest_edges, n);
    if (out.forest_edges) {
        size_t sort_bytes = 0;
        HIPC(rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)w.d_forest[0], (unsigned long long *)w.d_forest[1], out.forest_edges, 0, 64, c->stream));
        F2VC(w.d_sort.reserve(c, sort_bytes, kCcWhat));
        HIPC(rocprim::radix_sort_keys((void *)(uint8_t *)w.d_sort, sort_bytes, (unsigned long long *)w.d_forest[0], (unsigned long long *)w.d_forest[1], out.forest_edges, 0,
                                      64, c->stream));
    }
    F2VC(w.timer.stop(c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&out.seconds));
    return F2V_OK;
}

int forest_flags(f2v_ctx *c, const char *who, uint64_t seed, double *seconds) {
    (void)who;
    f2v_ctx::Components &w = c->cc;
    if (w.flag_valid && w.flag_seed == seed && w.flag_bits == w.key_bits) return F2V_OK;  // (the CSR of a handle never changes)
    w.flag_valid = false;
    ForestRun run;
    F2VC(forest_run(c, seed, 1, run));
    F2VC(w.d_flag.reserve(c, std::max<uint64_t>(c->nnz, 1), kCcWhat));
    CcArgs a;
    F2VC(cc_prepare(c, a));
    a.forest = w.d_forest[1];
    a.forest_count = run.forest_edges;
    a.flag = w.d_flag;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(forest_mark_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    *seconds += run.seconds;
    F2VC(w.timer.seconds(seconds));
    w.flag_valid = true;
    w.flag_seed = seed;
    w.flag_bits = w.key_bits;
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_components(f2v_handle c, uint32_t *labels_out, uint32_t *sizes_out, f2v_components_t *info) {
    if (!c || !labels_out || !info) return fail(F2V_EINVAL, "f2v_components: null argument");
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_components: the CSR's column ids are not ascending inside every row (needed to search a row)");
    HIPC(hipSetDevice(c->device));
    *info = f2v_components_t{};
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;
    f2v_ctx::Components &w = c->cc;
    CcArgs a;
    F2VC(cc_prepare(c, a));
    F2VC(w.d_size.reserve(c, n, kCcWhat));
    F2VC(w.d_sizes.reserve(c, n, kCcWhat));
    a.size = w.d_size;
    a.sizes_out = w.d_sizes;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(cc_iota_kernel, cc_grid(n), dim3(256), 0, c->stream, (uint32_t *)w.d_L, (uint32_t *)w.d_P, n);
    hipLaunchKernelGGL(cc_edges_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    uint32_t rounds = 0;
    for (;;) {
        hipLaunchKernelGGL(cc_hook_kernel, cc_piece_grid(a), dim3(256), 0, c->stream, a);
        bool hooked = false;
        F2VC(cc_flatten(c, a, &hooked));
        rounds++;
        if (!hooked) break;
    }
    HIPC(hipMemsetAsync(w.d_size, 0, (size_t)n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(cc_size_kernel, cc_grid(n), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(cc_stat_kernel, cc_grid(n), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long sums[8];
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(labels_out, w.d_L, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (sizes_out) HIPC(hipMemcpyAsync(sizes_out, w.d_sizes, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&info->seconds));
    info->edges = sums[2];
    info->components = (uint32_t)sums[3];
    info->isolated = (uint32_t)sums[4];
    info->largest = (uint32_t)(sums[5] >> 32);
    info->largest_label = 0xFFFFFFFFu - (uint32_t)sums[5];
    info->rounds = rounds;
    return F2V_OK;
}

int f2v_spanning_forest(f2v_handle c, uint64_t seed, uint32_t greatest, uint32_t *u_out, uint32_t *v_out, uint64_t cap, uint64_t *count_out, f2v_forest_t *info) {
    if (!c || !count_out) return fail(F2V_EINVAL, "f2v_spanning_forest: null argument");
    if ((u_out != nullptr) != (v_out != nullptr)) return fail(F2V_EINVAL, "f2v_spanning_forest: u_out and v_out are given together or not at all");
    if (greatest > 1) return fail(F2V_EINVAL, "f2v_spanning_forest: greatest = %u is neither 0 nor 1", greatest);
    if (!rows_ascending(c)) return fail(F2V_EINVAL, "f2v_spanning_forest: the CSR's column ids are not ascending inside every row (needed to search a row)");
    HIPC(hipSetDevice(c->device));
    *count_out = 0;
    if (info) *info = f2v_forest_t{};
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;
    ForestRun run;
    F2VC(forest_run(c, seed, greatest, run));
    *count_out = run.forest_edges;
    if (info) {
        info->seconds = run.seconds;
        info->edges = run.edges;
        info->forest_edges = run.forest_edges;
        info->components = n - (uint32_t)run.forest_edges;
        info->rounds = run.rounds;
    }
    if (!u_out) return F2V_OK;
    if (cap < run.forest_edges)
        return fail(F2V_EINVAL, "f2v_spanning_forest: the forest has %llu pairs, the arrays hold %llu", (unsigned long long)run.forest_edges, (unsigned long long)cap);
    std::vector<unsigned long long> pairs(run.forest_edges);
    if (run.forest_edges) {
        HIPC(hipMemcpyAsync(pairs.data(), c->cc.d_forest[1], run.forest_edges * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    for (uint64_t i = 0; i < run.forest_edges; i++) {
        u_out[i] = (uint32_t)(pairs[i] >> 32);
        v_out[i] = (uint32_t)pairs[i];
    }
    return F2V_OK;
}

int f2v_forest_round_seconds(f2v_handle c, double *seconds_out, uint32_t cap, uint32_t *count_out) {
    if (!c || !count_out) return fail(F2V_EINVAL, "f2v_forest_round_seconds: null argument");
    const std::vector<double> &r = c->cc.round_seconds;
    *count_out = (uint32_t)r.size();
    if (seconds_out)
        for (uint32_t i = 0; i < cap && i < r.size(); i++) seconds_out[i] = r[i];
    return F2V_OK;
}

int f2v_subgraph(f2v_handle c, const uint8_t *keep, uint32_t *rowptr_out, uint32_t *colids_out, uint64_t cap, uint32_t *new_id_out, uint32_t *rows_out,
                 uint64_t *nnz_out) {
    if (!c || !keep || !rows_out || !nnz_out) return fail(F2V_EINVAL, "f2v_subgraph: null argument");
    if ((rowptr_out != nullptr) != (colids_out != nullptr)) return fail(F2V_EINVAL, "f2v_subgraph: rowptr_out and colids_out are given together or not at all");
    HIPC(hipSetDevice(c->device));
    *rows_out = 0;
    *nnz_out = 0;
    const uint32_t n = c->n;
    if (n == 0) return F2V_OK;
    f2v_ctx::Components &w = c->cc;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kLinkScanTile - 1) / kLinkScanTile), rows = std::min((n + 3) / 4, 8192u);
    F2VC(w.d_keep.reserve(c, n, kCcWhat));
    F2VC(w.d_kept.reserve(c, n, kCcWhat));
    F2VC(w.d_cnt.reserve(c, n, kCcWhat));
    F2VC(w.d_zero.reserve(c, n, kCcWhat));
    F2VC(w.d_id_at.reserve(c, n, kCcWhat));
    F2VC(w.d_row_at.reserve(c, n, kCcWhat));
    F2VC(w.d_tile.reserve(c, tiles, kCcWhat));
    F2VC(w.d_sums.reserve(c, 8, kCcWhat));
    SubArgs a{};
    a.rowptr = c->d_rowptr;
    a.colids = c->d_colids;
    a.keep = w.d_keep;
    a.kept = w.d_kept;
    a.cnt = w.d_cnt;
    a.id_at = w.d_id_at;
    a.row_at = w.d_row_at;
    a.sums = w.d_sums;
    a.n = n;
    LinkArgs l{};  // the 64-bit exclusive prefix sum of f2v_linkpairs.hip.h
    l.n = n;
    l.tile = w.d_tile;
    l.total = w.d_zero;
    HIPC(hipMemcpyAsync(w.d_keep, keep, n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(w.d_sums, 0, 8 * sizeof(unsigned long long), c->stream));
    HIPC(hipMemsetAsync(w.d_zero, 0, (size_t)n * sizeof(uint32_t), c->stream));
    auto scan = [&](uint32_t *p, unsigned long long *offset) {
        l.p = p;
        l.offset = offset;
        hipLaunchKernelGGL(link_scan_tile_kernel, dim3(tiles), dim3(256), 0, c->stream, l);
        hipLaunchKernelGGL(link_scan_top_kernel, dim3(1), dim3(256), 0, c->stream, l, tiles);
        hipLaunchKernelGGL(link_scan_apply_kernel, dim3(tiles), dim3(256), 0, c->stream, l);
    };
    double seconds = 0.0;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(sub_count_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    scan(w.d_kept, w.d_id_at);
    scan(w.d_cnt, w.d_row_at);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    unsigned long long sums[2];
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    c->cc_subgraph_seconds = seconds;
    *rows_out = (uint32_t)sums[0];
    *nnz_out = sums[1];
    if (!rowptr_out) return F2V_OK;
    if (cap < sums[1]) return fail(F2V_EINVAL, "f2v_subgraph: the subgraph has %llu nonzeros, colids_out holds %llu", sums[1], (unsigned long long)cap);
    F2VC(w.d_rowptr.reserve(c, (size_t)sums[0] + 1, kCcWhat));
    F2VC(w.d_colids.reserve(c, std::max<uint64_t>(sums[1], 1), kCcWhat));
    F2VC(w.d_newid.reserve(c, n, kCcWhat));
    a.rowptr_out = w.d_rowptr;
    a.colids_out = w.d_colids;
    a.new_id = w.d_newid;
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(sub_fill_kernel, dim3(rows), dim3(256), 0, c->stream, a);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    if (sums[0]) HIPC(hipMemcpyAsync(rowptr_out, w.d_rowptr, (size_t)sums[0] * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (sums[1]) HIPC(hipMemcpyAsync(colids_out, w.d_colids, (size_t)sums[1] * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (new_id_out) HIPC(hipMemcpyAsync(new_id_out, w.d_newid, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(w.timer.seconds(&seconds));
    c->cc_subgraph_seconds = seconds;
    rowptr_out[sums[0]] = (uint32_t)sums[1];
    return F2V_OK;
}

}  // extern "C"

// ---- t-SNE layout (f2v_tsne.hip.h; definition in include/f2v.h) -------------------------------------------------------------------
namespace {

// The two calls' checks on the sample -- `sid` receives it, every vertex where sample_ids is NULL -- then settled_enter
int tsne_enter(f2v_ctx *c, const char *who, const uint32_t *sample_ids, uint32_t m, std::vector<uint32_t> &sid) {
    const uint32_t n = c->n;
    if (!sample_ids) m = n;
    if (m < 8) return fail(F2V_EINVAL, "%s: %u points are fewer than 8", who, m);
    if (m > n) return fail(F2V_EINVAL, "%s: %u samples of %u vertices hold a duplicate", who, m, n);
    sid.resize(m);
    std::vector<bool> seen(n, false);
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t v = sample_ids ? sample_ids[i] : i;
        if (v >= n) return fail(F2V_EINVAL, "%s: sample %u names vertex %u of %u", who, i, v, n);
        if (seen[v]) return fail(F2V_EINVAL, "%s: sample %u names vertex %u a second time", who, i, v);
        seen[v] = true;
        sid[i] = v;
    }
    return settled_enter(c, who);
}

// k = floor(3 perplexity) and its range
int tsne_neighbours(const char *who, double perplexity, uint32_t m, uint32_t *k) {
    if (!(perplexity > 1.0)) return fail(F2V_EINVAL, "%s: the perplexity must be a number above 1", who);
    const double k3 = std::floor(3.0 * perplexity);
    if (k3 > (double)F2V_NEAREST_MAX_K) return fail(F2V_EINVAL, "%s: floor(3 x perplexity) is above %d neighbours", who, F2V_NEAREST_MAX_K);
    if (k3 >= (double)m) return fail(F2V_EINVAL, "%s: floor(3 x perplexity) = %u neighbours need more than %u points", who, (uint32_t)k3, m);
    *k = (uint32_t)k3;
    return F2V_OK;
}

// The symmetric P of the sample on the host: the rows gathered, their k nearest among themselves by the nearest-neighbour kernels as
// they are, the conditional affinities on the device, the symmetric sum on the host.  *seconds += the device time of the launches.
int tsne_affinities_host(f2v_ctx *c, const std::vector<uint32_t> &sid, uint32_t k, double perplexity, std::vector<uint32_t> &rowptr,
                         std::vector<uint32_t> &colids, std::vector<double> &values, double *seconds) {
    f2v_ctx::Tsne &w = c->ts;
    const uint32_t m = (uint32_t)sid.size(), D = c->D;
    const size_t slots = (size_t)m * k;
    const char *what = "t-SNE";
    F2VC(w.d_sid.reserve(c, m, what));
    F2VC(w.d_G.reserve(c, (size_t)m * D, what));
    F2VC(w.d_nbr.reserve(c, slots, what));
    F2VC(w.d_dist.reserve(c, slots, what));
    F2VC(w.d_cond.reserve(c, slots, what));
    HIPC(hipMemcpyAsync(w.d_sid, sid.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(nearest_gather_kernel, dim3(std::min<size_t>(((size_t)m * D + 255) / 256, 4096)), dim3(256), 0, c->stream, (const float *)c->d_X[c->cur],
                       (const uint32_t *)w.d_sid, m, D, w.d_G);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    std::vector<uint32_t> nbr(slots);
    double sec = 0.0;
    F2VC(nearest_run_on(c, w.d_G, D, nullptr, true, nullptr, m, k, F2V_SIM_L2, F2V_NEAREST_EXCLUDE_SELF, nbr.data(), nullptr, nullptr, &sec, w.d_nbr, w.d_dist, m));
    *seconds += sec;
    F2VC(w.timer.seconds(seconds));  // (the queries have synchronised the stream)
    F2VC(w.timer.start(c->stream));
    hipLaunchKernelGGL(tsne_calibrate_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, (const float *)w.d_dist, m, k, perplexity, w.d_cond);
    HIPC(hipGetLastError());
    F2VC(w.timer.stop(c->stream));
    std::vector<double> cond(slots);
    HIPC(hipMemcpyAsync(cond.data(), w.d_cond, slots * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "t-SNE affinities"));
    F2VC(w.timer.seconds(seconds));
    for (size_t e = 0; e < slots; e++)
        if (nbr[e] >= m) return fail(F2V_EINVAL, "t-SNE affinities: point %zu has fewer than %u neighbours", e / k, k);
    tsne_symmetrize_host(nbr.data(), cond.data(), m, k, rowptr, colids, values);
    return F2V_OK;
}

template <int D2, int ROWS>
void launch_tsne_pair_t(f2v_ctx *c, const TsnePairArgs &a, uint32_t slices) {
    hipLaunchKernelGGL((tsne_pair_kernel<D2, ROWS>), dim3((a.m + ROWS - 1) / ROWS, slices), dim3(ROWS), 0, c->stream, a);
}

template <int D2>
void launch_tsne_pair(f2v_ctx *c, const TsnePairArgs &a, uint32_t rows, uint32_t slices) {
    if (rows == 64) launch_tsne_pair_t<D2, 64>(c, a, slices);
    else if (rows == 128) launch_tsne_pair_t<D2, 128>(c, a, slices);
    else launch_tsne_pair_t<D2, 256>(c, a, slices);
}

}  // namespace

extern "C" {

int f2v_tsne_affinities(f2v_handle c, const uint32_t *sample_ids, uint32_t m, double perplexity, uint32_t *rowptr_out, uint32_t *colids_out,
                        double *values_out, uint64_t cap, uint64_t *nnz_out, double *seconds_out) {
    if (!c || !rowptr_out || !colids_out || !values_out || !nnz_out) return fail(F2V_EINVAL, "f2v_tsne_affinities: null argument");
    if (!sample_ids) m = c->n;
    uint32_t k = 0;
    if (m >= 8) F2VC(tsne_neighbours("f2v_tsne_affinities", perplexity, m, &k));
    std::vector<uint32_t> sid, rowptr, colids;
    std::vector<double> values;
    F2VC(tsne_enter(c, "f2v_tsne_affinities", sample_ids, m, sid));
    double seconds = 0.0;
    F2VC(tsne_affinities_host(c, sid, k, perplexity, rowptr, colids, values, &seconds));
    *nnz_out = colids.size();
    if (seconds_out) *seconds_out = seconds;
    if (colids.size() > cap) return fail(F2V_EINVAL, "f2v_tsne_affinities: %zu entries need more room than cap = %llu", colids.size(), (unsigned long long)cap);
    memcpy(rowptr_out, rowptr.data(), rowptr.size() * sizeof(uint32_t));
    memcpy(colids_out, colids.data(), colids.size() * sizeof(uint32_t));
    memcpy(values_out, values.data(), values.size() * sizeof(double));
    return F2V_OK;
}

int f2v_tsne(f2v_handle c, const uint32_t *sample_ids, uint32_t m, uint32_t d2, const f2v_tsne_params *params, const uint32_t *p_rowptr,
             const uint32_t *p_colids, const double *p_values, const double *y_init, float *y_out, f2v_tsne_t *info) {
    const char *who = "f2v_tsne";
    if (!c || !y_out || !info) return fail(F2V_EINVAL, "f2v_tsne: null argument");
    if (d2 != 2 && d2 != 3) return fail(F2V_EINVAL, "f2v_tsne: d2 = %u is neither 2 nor 3", d2);
    f2v_tsne_params p{};
    if (params) p = *params;
    if (!(p.perplexity >= 0.0) || !(p.exaggeration >= 0.0) || !(p.learning_rate >= 0.0) || p.exaggeration > 1e300 || p.learning_rate > 1e300)
        return fail(F2V_EINVAL, "f2v_tsne: a parameter is negative or not a number");
    if (p.perplexity == 0.0) p.perplexity = 30.0;
    if (p.exaggeration == 0.0) p.exaggeration = 12.0;
    if (p.iters == 0) p.iters = 1000;
    if (p.exaggeration_iters == 0) p.exaggeration_iters = 250;
    const bool given = p_rowptr || p_colids || p_values;
    if (given && !(p_rowptr && p_colids && p_values)) return fail(F2V_EINVAL, "f2v_tsne: P is given in part (row pointers, column ids and values go together)");
    if (!sample_ids) m = c->n;
    uint32_t k = 0;
    if (!given && m >= 8) F2VC(tsne_neighbours(who, p.perplexity, m, &k));
    if (given && m >= 8) {
        if (p_rowptr[0] != 0) return fail(F2V_EINVAL, "f2v_tsne: P's row pointers do not start at 0");
        for (uint32_t i = 0; i < m; i++) {
            if (p_rowptr[i + 1] < p_rowptr[i]) return fail(F2V_EINVAL, "f2v_tsne: P's row pointers descend at row %u", i);
            for (uint32_t e = p_rowptr[i]; e < p_rowptr[i + 1]; e++) {
                if (p_colids[e] >= m) return fail(F2V_EINVAL, "f2v_tsne: row %u of P names column %u of %u", i, p_colids[e], m);
                if (e > p_rowptr[i] && p_colids[e] <= p_colids[e - 1]) return fail(F2V_EINVAL, "f2v_tsne: the column ids of row %u of P do not ascend", i);
                if (!(p_values[e] >= 2.2250738585072014e-308 && p_values[e] <= 1.7976931348623157e308))
                    return fail(F2V_EINVAL, "f2v_tsne: entry %u of P is not a positive normal number", e);
            }
        }
    }
    std::vector<uint32_t> sid, rowptr, colids;
    std::vector<double> values;
    F2VC(tsne_enter(c, who, sample_ids, m, sid));
    f2v_ctx::Tsne &w = c->ts;
    w.kl_iters.clear();
    w.kl_values.clear();
    const uint32_t n = c->n;
    double seconds = 0.0;
    if (!given) {
        F2VC(tsne_affinities_host(c, sid, k, p.perplexity, rowptr, colids, values, &seconds));
        p_rowptr = rowptr.data();
        p_colids = colids.data();
        p_values = values.data();
    }
    const size_t nnz = p_rowptr[m], cells = (size_t)m * d2;
    // the start: Y, update = 0, gains = 1 and yf
    std::vector<double> state(3 * cells, 0.0);
    if (y_init) {
        memcpy(state.data(), y_init, cells * sizeof(double));
    } else {
        std::vector<float> proj((size_t)n * d2);
        double var[3] = {0.0, 0.0, 0.0};
        f2v_pca_t pi{};
        F2VC(f2v_pca(c, d2, proj.data(), nullptr, nullptr, var, &pi));
        if (!(var[0] > 0.0)) return fail(F2V_EINVAL, "f2v_tsne: the matrix's first principal component has no variance: give y_init");
        const double scale = 1e-4 / std::sqrt(var[0]);
        for (uint32_t i = 0; i < m; i++)
            for (uint32_t d = 0; d < d2; d++) state[(size_t)i * d2 + d] = (double)proj[(size_t)sid[i] * d2 + d] * scale;
    }
    std::vector<float> yf(cells);
    for (size_t i = 0; i < cells; i++) {
        yf[i] = (float)state[i];
        state[2 * cells + i] = 1.0;
    }
    const double lr = p.learning_rate > 0.0 ? p.learning_rate : std::max((double)m / p.exaggeration / 4.0, 50.0);
    const uint32_t spans = (m + kTsneSpanCols - 1) / kTsneSpanCols, pieces = (m + kTsnePiece - 1) / kTsnePiece;
    const uint32_t logged = p.kl_every ? p.iters / p.kl_every : 0;
    const char *what = "t-SNE";
    F2VC(w.d_prow.reserve(c, (size_t)m + 1, what));
    F2VC(w.d_pcol.reserve(c, nnz, what));
    F2VC(w.d_pval.reserve(c, nnz, what));
    F2VC(w.d_state.reserve(c, 3 * cells, what));
    F2VC(w.d_yf.reserve(c, 2 * cells, what));
    F2VC(w.d_ws.reserve(c, (size_t)spans * (1 + d2) * m, what));
    F2VC(w.d_part.reserve(c, pieces, what));
    F2VC(w.d_out.reserve(c, (size_t)logged + 2, what));
    HIPC(hipMemcpyAsync(w.d_prow, p_rowptr, ((size_t)m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_pcol, p_colids, nnz * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_pval, p_values, nnz * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_state, state.data(), 3 * cells * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_yf, yf.data(), cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
    // placement (tools/tsne_time.py): 256 rows per workgroup from 4096 points on, and one span per workgroup -- the most wavefronts;
    // several spans per workgroup were slower at every size measured
    const uint32_t rows = w.rows ? w.rows : (m < 4096 ? 64u : 256u);
    const uint32_t per_slice = std::min(spans, w.slices ? w.slices : 1u);
    const uint32_t slices = (spans + per_slice - 1) / per_slice;
    float *yfb[2] = {w.d_yf, w.d_yf + cells};
    double *Z = w.d_out;  // d_out: Z, the logged KL values, the final KL
    auto pair_z = [&](const float *y) {
        TsnePairArgs a{y, w.d_ws, m, spans, per_slice};
        if (d2 == 2) launch_tsne_pair<2>(c, a, rows, slices);
        else launch_tsne_pair<3>(c, a, rows, slices);
        hipLaunchKernelGGL(tsne_zpiece_kernel, dim3(pieces), dim3(64), 0, c->stream, (const double *)w.d_ws, m, spans, d2, w.d_part);
        hipLaunchKernelGGL(tsne_seqsum_kernel, dim3(1), dim3(64), 0, c->stream, (const double *)w.d_part, pieces, Z);
    };
    auto kl = [&](const float *y, double *out) {
        TsneKlArgs a{Z, w.d_prow, w.d_pcol, w.d_pval, y, w.d_part, m};
        if (d2 == 2) hipLaunchKernelGGL(tsne_kl_kernel<2>, dim3(pieces), dim3(64), 0, c->stream, a);
        else hipLaunchKernelGGL(tsne_kl_kernel<3>, dim3(pieces), dim3(64), 0, c->stream, a);
        hipLaunchKernelGGL(tsne_seqsum_kernel, dim3(1), dim3(64), 0, c->stream, (const double *)w.d_part, pieces, out);
    };
    F2VC(w.timer.start(c->stream));
    int cur = 0;
    bool fresh = false;  // the span sums and Z are those of yfb[cur]
    for (uint32_t it = 0; it < p.iters; it++) {
        if (!fresh) pair_z(yfb[cur]);
        const bool early = it < p.exaggeration_iters;
        TsneStepArgs a{};
        a.ws = w.d_ws;
        a.Z = Z;
        a.rowptr = w.d_prow;
        a.colids = w.d_pcol;
        a.values = w.d_pval;
        a.yf_in = yfb[cur];
        a.yf_out = yfb[cur ^ 1];
        a.y = w.d_state;
        a.update = w.d_state + cells;
        a.gains = w.d_state + 2 * cells;
        a.m = m;
        a.spans = spans;
        a.ex = early ? p.exaggeration : 1.0;
        a.momentum = early ? 0.5 : 0.8;
        a.lr = lr;
        if (d2 == 2) hipLaunchKernelGGL(tsne_step_kernel<2>, dim3((m + 3) / 4), dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL(tsne_step_kernel<3>, dim3((m + 3) / 4), dim3(256), 0, c->stream, a);
        cur ^= 1;
        fresh = false;
        const bool last = it + 1 == p.iters, log = p.kl_every && (it + 1) % p.kl_every == 0;
        if (last || log) {
            pair_z(yfb[cur]);
            fresh = true;
            if (log) {
                kl(yfb[cur], w.d_out + 1 + w.kl_iters.size());
                w.kl_iters.push_back(it + 1);
            }
            if (last) kl(yfb[cur], w.d_out + 1 + logged);
        }
        HIPC(hipGetLastError());
    }
    F2VC(w.timer.stop(c->stream));
    std::vector<double> out((size_t)logged + 2);
    HIPC(hipMemcpyAsync(out.data(), w.d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(y_out, yfb[cur], cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, who));
    F2VC(w.timer.seconds(&seconds));
    w.kl_values.assign(out.begin() + 1, out.begin() + 1 + w.kl_iters.size());
    info->kl = out[1 + logged];
    info->z = out[0];
    info->learning_rate = lr;
    info->seconds = seconds;
    info->nnz = nnz;
    info->k = k;
    info->reserved = 0;
    return F2V_OK;
}

int f2v_tsne_kl_log(f2v_handle c, uint32_t *iterations_out, double *values_out, uint32_t cap, uint32_t *count_out) {
    if (!c || !count_out || (cap && (!iterations_out || !values_out))) return fail(F2V_EINVAL, "f2v_tsne_kl_log: null argument");
    const uint32_t count = (uint32_t)c->ts.kl_values.size();  // (empty after a call that failed)
    for (uint32_t i = 0; i < count && i < cap; i++) {
        iterations_out[i] = c->ts.kl_iters[i];
        values_out[i] = c->ts.kl_values[i];
    }
    *count_out = count;
    return F2V_OK;
}

}  // extern "C"

// ---- layout (f2v_layout.hip.h; definition in include/f2v.h) -----------------------------------------------------------------------
namespace {

// The layout calls' range check on n (their kernels count pieces in 32 bits), then settled_enter
int lay_enter(f2v_ctx *c, const char *who) {
    if (c->n >= 0xFFFFFFFFu - kPcaPiece) return fail(F2V_EINVAL, "%s: too many vertices for 32-bit pieces", who);
    return settled_enter(c, who);
}

// The mean (lay.d_mean, D doubles) and the packed upper triangle of the scatter matrix (lay.d_S) of the settled matrix, enqueued on
// the handle's stream: column sums and chains per piece of 4096 vertices, the pieces added in order.
int pca_moments(f2v_ctx *c) {
    f2v_ctx::Layout &w = c->lay;
    const uint32_t n = c->n, D = c->D, pieces = (n + kPcaPiece - 1) / kPcaPiece, tiles = (D + kPcaTile - 1) / kPcaTile;
    const size_t width = (size_t)D * (D + 1) / 2;
    F2VC(w.d_ws.reserve(c, (size_t)pieces * width, "layout"));
    F2VC(w.d_mean.reserve(c, D, "layout"));
    F2VC(w.d_S.reserve(c, width, "layout"));
    const float *X = c->d_X[c->cur];
    hipLaunchKernelGGL(pca_colsum_kernel, dim3(pieces, (D + 63) / 64), dim3(64), 0, c->stream, X, n, D, w.d_ws);
    hipLaunchKernelGGL(pca_reduce_kernel, dim3((D + 255) / 256), dim3(256), 0, c->stream, (const double *)w.d_ws, pieces, (size_t)D, (double)n, w.d_mean);
    PcaScatterArgs a{};
    a.X = X;
    a.mean = w.d_mean;
    a.ws = w.d_ws;
    a.width = width;
    a.n = n;
    a.D = D;
    a.tiles = tiles;
    hipLaunchKernelGGL(pca_scatter_kernel, dim3(pieces, tiles * (tiles + 1) / 2), dim3(kPcaThreads), 0, c->stream, a);
    hipLaunchKernelGGL(pca_reduce_kernel, dim3((uint32_t)((width + 255) / 256)), dim3(256), 0, c->stream, (const double *)w.d_ws, pieces, width, 1.0, w.d_S);
    HIPC(hipGetLastError());
    return F2V_OK;
}

// mean and the full symmetric scatter matrix on the host (and the device time of their launches)
int pca_moments_host(f2v_ctx *c, std::vector<double> &mean, std::vector<double> &S, double *seconds) {
    f2v_ctx::Layout &w = c->lay;
    const uint32_t D = c->D;
    const size_t width = (size_t)D * (D + 1) / 2;
    F2VC(w.timer.start(c->stream));
    F2VC(pca_moments(c));
    F2VC(w.timer.stop(c->stream));
    std::vector<double> packed(width);
    mean.resize(D);
    HIPC(hipMemcpyAsync(mean.data(), w.d_mean, (size_t)D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(packed.data(), w.d_S, width * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "f2v_pca"));
    S.resize((size_t)D * D);
    for (uint32_t d = 0; d < D; d++)
        for (uint32_t e = d; e < D; e++) S[(size_t)d * D + e] = S[(size_t)e * D + d] = packed[pca_packed(D, d, e)];
    *seconds = 0.0;
    return w.timer.seconds(seconds);
}

template <int RB>
int launch_rank_t(f2v_ctx *c, TrustRankArgs a, uint32_t spans) {
    a.blocks = (a.nq + RB - 1) / RB;
    const size_t lds = trust_lds_bytes(RB, a.k);  // a sample block's thresholds and counts live in LDS: up to 114 KB at k = 128
    F2VC(allow_lds(c, reinterpret_cast<const void *>(&trust_rank_kernel<RB>), lds));
    hipLaunchKernelGGL((trust_rank_kernel<RB>), dim3(spans * a.blocks), dim3(kSepThreads), lds, c->stream, a);
    HIPC(hipGetLastError());
    return F2V_OK;
}

}  // namespace

extern "C" {

int f2v_pca(f2v_handle c, uint32_t d2, float *y_out, double *components_out, double *mean_out, double *variance_out, f2v_pca_t *info) {
    if (!c || !info) return fail(F2V_EINVAL, "f2v_pca: null argument");
    if (d2 == 0 || d2 > c->D) return fail(F2V_EINVAL, "f2v_pca: d2 = %u is outside 1..dim = %u", d2, c->D);
    if (c->n < 2) return fail(F2V_EINVAL, "f2v_pca: a graph of %u vertices has no variance", c->n);
    F2VC(lay_enter(c, "f2v_pca"));
    f2v_ctx::Layout &w = c->lay;
    const uint32_t n = c->n, D = c->D;
    std::vector<double> mean, A, V((size_t)D * D);
    double seconds = 0.0;
    F2VC(pca_moments_host(c, mean, A, &seconds));
    double trace = 0.0;
    for (uint32_t d = 0; d < D; d++) trace += A[(size_t)d * D + d];
    uint32_t sweeps = 0, converged = 0;
    pca_jacobi_host(A.data(), V.data(), D, &sweeps, &converged);
    // eigenvalue descending, ties by ascending column (a NaN after every number)
    std::vector<uint32_t> order(D);
    for (uint32_t d = 0; d < D; d++) order[d] = d;
    auto lam = [&](uint32_t j) { return A[(size_t)j * D + j]; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const double lx = lam(x), ly = lam(y);
        if (lx != lx || ly != ly) return ly != ly && lx == lx;
        return lx > ly;
    });
    std::vector<double> W((size_t)d2 * D);
    for (uint32_t k = 0; k < d2; k++) {
        uint32_t big = 0;
        for (uint32_t d = 0; d < D; d++) {
            W[(size_t)k * D + d] = V[(size_t)d * D + order[k]];
            if (std::fabs(W[(size_t)k * D + d]) > std::fabs(W[(size_t)k * D + big])) big = d;
        }
        if (W[(size_t)k * D + big] < 0.0)
            for (uint32_t d = 0; d < D; d++) W[(size_t)k * D + d] = -W[(size_t)k * D + d];
    }
    if (y_out) {
        F2VC(w.d_W.reserve(c, (size_t)d2 * D, "layout"));
        F2VC(w.d_P.reserve(c, (size_t)n * d2, "layout"));
        HIPC(hipMemcpyAsync(w.d_W, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        F2VC(w.timer.start(c->stream));
        hipLaunchKernelGGL(pca_project_kernel, dim3((uint32_t)(((size_t)n * d2 + 255) / 256)), dim3(256), 0, c->stream, (const float *)c->d_X[c->cur],
                           (const double *)w.d_mean, (const double *)w.d_W, n, D, d2, w.d_P);
        HIPC(hipGetLastError());
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(y_out, w.d_P, (size_t)n * d2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(check_kernel_err(c, "f2v_pca"));
        F2VC(w.timer.seconds(&seconds));
    }
    if (components_out) memcpy(components_out, W.data(), W.size() * sizeof(double));
    if (mean_out) memcpy(mean_out, mean.data(), (size_t)D * sizeof(double));
    for (uint32_t k = 0; variance_out && k < d2; k++) variance_out[k] = lam(order[k]) / (double)(n - 1);
    info->total_variance = trace / (double)(n - 1);
    info->seconds = seconds;
    info->sweeps = sweeps;
    info->converged = converged;
    return F2V_OK;
}

int f2v_trustworthiness(f2v_handle c, const float *Y, uint32_t d2, uint32_t k, const uint32_t *sample_ids, uint32_t nq, uint64_t *penalty_x_out,
                        uint64_t *penalty_y_out, f2v_trust_t *out) {
    if (!c || !Y || !out) return fail(F2V_EINVAL, "f2v_trustworthiness: null argument");
    if (d2 == 0 || d2 > F2V_TRUST_MAX_DIM) return fail(F2V_EINVAL, "f2v_trustworthiness: d2 = %u is outside 1..%d", d2, F2V_TRUST_MAX_DIM);
    if (k == 0 || k > F2V_NEAREST_MAX_K) return fail(F2V_EINVAL, "f2v_trustworthiness: k = %u is outside 1..%d", k, F2V_NEAREST_MAX_K);
    if (2 * (uint64_t)k >= c->n) return fail(F2V_EINVAL, "f2v_trustworthiness: k = %u must be below n / 2 = %u / 2", k, c->n);
    if (sample_ids && nq == 0) return fail(F2V_EINVAL, "f2v_trustworthiness: nq = 0 samples");
    const uint32_t n = c->n, D = c->D;
    if (!sample_ids) nq = n;
    std::vector<uint32_t> sid(nq);
    for (uint32_t i = 0; i < nq; i++) {
        sid[i] = sample_ids ? sample_ids[i] : i;
        if (sid[i] >= n) return fail(F2V_EINVAL, "f2v_trustworthiness: sample %u names vertex %u of %u", i, sid[i], n);
    }
    F2VC(lay_enter(c, "f2v_trustworthiness"));
    f2v_ctx::Layout &w = c->lay;
    const uint32_t chunk = std::min(w.chunk, nq), rb = w.block == 128 && k <= 32 ? 128u : 64u;
    const char *what = "layout";
    F2VC(w.d_Y.reserve(c, (size_t)n * d2, what));
    F2VC(w.d_sid.reserve(c, nq, what));
    F2VC(w.d_nx.reserve(c, (size_t)chunk * k, what));
    F2VC(w.d_ny.reserve(c, (size_t)chunk * k, what));
    F2VC(w.d_thr.reserve(c, (size_t)chunk * k, what));
    F2VC(w.d_hist.reserve(c, (size_t)chunk * k, what));
    F2VC(w.d_pen.reserve(c, 2 * (size_t)nq, what));
    F2VC(w.d_sums.reserve(c, 3, what));
    HIPC(hipMemcpyAsync(w.d_Y, Y, (size_t)n * d2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(w.d_sid, sid.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(w.d_sums, 0, 3 * sizeof(unsigned long long), c->stream));
    const float *X = c->d_X[c->cur];
    double seconds = 0.0;
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cq = std::min(chunk, nq - q0), blocks = (cq + rb - 1) / rb;
        // the k nearest in both spaces, by the nearest-neighbour kernels as they are
        double sec = 0.0;
        F2VC(nearest_run_on(c, X, D, sid.data() + q0, false, nullptr, cq, k, F2V_SIM_L2, F2V_NEAREST_EXCLUDE_SELF, nullptr, nullptr, nullptr, &sec, w.d_nx));
        seconds += sec;
        F2VC(nearest_run_on(c, w.d_Y, d2, sid.data() + q0, false, nullptr, cq, k, F2V_SIM_L2, F2V_NEAREST_EXCLUDE_SELF, nullptr, nullptr, nullptr, &sec, w.d_ny));
        seconds += sec;
        // candidates per workgroup: enough workgroups for every CU a few times over (placement only: the counts add up exactly)
        const uint32_t want = std::max(1u, 2048u / blocks);
        uint32_t span = ((n + want - 1) / want + 63u) / 64u * 64u;
        span = std::min(std::max(span, 256u), kTrustMaxSpan);
        const uint32_t spans = (n + span - 1) / span;
        if ((uint64_t)spans * blocks > 0x7FFFFFFFull) return fail(F2V_EINVAL, "f2v_trustworthiness: too many workgroups per launch: lower \"trust_chunk\"");
        F2VC(w.timer.start(c->stream));
        for (int dir = 0; dir < 2; dir++) {  // 0: the layout's neighbours ranked in X (trustworthiness), 1: X's neighbours ranked in Y (continuity)
            TrustKeyArgs ka{};
            ka.M = dir ? w.d_Y : X;
            ka.sid = w.d_sid + q0;
            ka.tgt = dir ? w.d_nx : w.d_ny;
            ka.own = dir ? w.d_ny : w.d_nx;
            ka.thr = w.d_thr;
            ka.hits = dir ? nullptr : w.d_sums + 2;
            ka.n = n;
            ka.D = dir ? d2 : D;
            ka.k = k;
            hipLaunchKernelGGL(trust_keys_kernel, dim3(cq), dim3(128), 0, c->stream, ka);
            HIPC(hipGetLastError());
            HIPC(hipMemsetAsync(w.d_hist, 0, (size_t)cq * k * sizeof(uint32_t), c->stream));
            TrustRankArgs ra{};
            ra.M = ka.M;
            ra.sid = ka.sid;
            ra.thr = w.d_thr;
            ra.hist = w.d_hist;
            ra.n = n;
            ra.D = ka.D;
            ra.nq = cq;
            ra.k = k;
            ra.span = span;
            F2VC(rb == 128 ? launch_rank_t<128>(c, ra, spans) : launch_rank_t<64>(c, ra, spans));
            hipLaunchKernelGGL(trust_finish_kernel, dim3((cq + 255) / 256), dim3(256), 0, c->stream, (const nn_key_t *)w.d_thr, (const uint32_t *)w.d_hist, cq, k,
                               w.d_pen + (size_t)dir * nq + q0, w.d_sums + dir);
            HIPC(hipGetLastError());
        }
        F2VC(w.timer.stop(c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    uint64_t sums[3] = {0, 0, 0};
    HIPC(hipMemcpyAsync(sums, w.d_sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    if (penalty_x_out) HIPC(hipMemcpyAsync(penalty_x_out, w.d_pen, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (penalty_y_out) HIPC(hipMemcpyAsync(penalty_y_out, w.d_pen + nq, (size_t)nq * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    F2VC(check_kernel_err(c, "f2v_trustworthiness"));
    const double scale = 2.0 / ((double)nq * k * (2.0 * n - 3.0 * k - 1.0));
    out->trustworthiness = 1.0 - (double)sums[0] * scale;
    out->continuity = 1.0 - (double)sums[1] * scale;
    out->overlap = (double)sums[2] / ((double)nq * k);
    out->seconds = seconds;
    out->penalty_x = sums[0];
    out->penalty_y = sums[1];
    out->hits = sums[2];
    return F2V_OK;
}

#ifdef F2V_TEST_HOOKS
int f2v_test_pca_scatter(f2v_handle c, double *mean_out, double *scatter_out) {
    if (!c || !mean_out || !scatter_out) return fail(F2V_EINVAL, "f2v_test_pca_scatter: null argument");
    F2VC(lay_enter(c, "f2v_test_pca_scatter"));
    std::vector<double> mean, S;
    double seconds = 0.0;
    F2VC(pca_moments_host(c, mean, S, &seconds));
    memcpy(mean_out, mean.data(), mean.size() * sizeof(double));
    memcpy(scatter_out, S.data(), S.size() * sizeof(double));
    return F2V_OK;
}
#endif

int f2v_logreg_eval(f2v_handle c, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const uint8_t *y, uint32_t classes,
                    const double *weights, double lambda, double *loss_out, double *grad_out, double *seconds_out) {
    if (!c || !a_ids || !y || !weights || !loss_out || !grad_out) return fail(F2V_EINVAL, "f2v_logreg_eval: null argument");
    if (!(lambda >= 0.0)) return fail(F2V_EINVAL, "f2v_logreg_eval: lambda must be a non-negative number");
    F2VC(logreg_enter(c, "f2v_logreg_eval", a_ids, b_ids, m, feature, y, classes));
    uint32_t cmap[F2V_LOGREG_MAX_CLASSES];
    for (uint32_t k = 0; k < classes; k++) cmap[k] = k;
    double seconds = 0.0;
    F2VC(logreg_pass(c, b_ids != nullptr, m, feature, classes, cmap, classes, weights, lambda, loss_out, grad_out, &seconds));
    F2VC(check_kernel_err(c, "f2v_logreg_eval"));
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

int f2v_logreg_fit(f2v_handle c, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const uint8_t *y, uint32_t classes,
                   double lambda, double tol, uint32_t max_iter, double *weights_out, f2v_logreg_t *info_out) {
    if (!c || !a_ids || !y || !weights_out || !info_out) return fail(F2V_EINVAL, "f2v_logreg_fit: null argument");
    if (!(lambda >= 0.0)) return fail(F2V_EINVAL, "f2v_logreg_fit: lambda must be a non-negative number");
    if (!(tol > 0.0)) return fail(F2V_EINVAL, "f2v_logreg_fit: tol must be positive");
    F2VC(logreg_enter(c, "f2v_logreg_fit", a_ids, b_ids, m, feature, y, classes));
    const uint32_t D = c->D, P = D + 1;
    const bool pairs = b_ids != nullptr;
    const double stop = tol * (double)m;
    std::vector<LbfgsClass> cls(classes);
    std::vector<uint32_t> cmap(classes);
    std::vector<double> W((size_t)classes * P, 0.0), loss(classes), grad((size_t)classes * P);
    double seconds = 0.0;
    for (uint32_t k = 0; k < classes; k++) cmap[k] = k;
    F2VC(logreg_pass(c, pairs, m, feature, classes, cmap.data(), classes, W.data(), lambda, loss.data(), grad.data(), &seconds));
    for (uint32_t k = 0; k < classes; k++) {
        LbfgsClass &s = cls[k];
        s.w.assign(P, 0.0);
        s.g.assign(grad.begin() + (size_t)k * P, grad.begin() + (size_t)(k + 1) * P);
        s.f = loss[k];
        s.evaluations = 1;
        s.gnorm = lr_norm_inf(s.g);
        s.converged = s.gnorm <= stop;
        s.active = !s.converged && max_iter > 0;
    }
    for (;;) {
        uint32_t nc = 0;
        for (uint32_t k = 0; k < classes; k++) {
            LbfgsClass &s = cls[k];
            if (!s.active) continue;
            if (!s.searching) {
                lbfgs_direction(s);
                double g1 = 0.0;
                for (double v : s.g) g1 += std::fabs(v);
                s.t = s.iterations == 0 ? 1.0 / g1 : 1.0;
                s.halvings = 0;
                s.searching = true;
            }
            s.trial.resize(P);
            for (uint32_t j = 0; j < P; j++) s.trial[j] = s.w[j] + s.t * s.p[j];
            std::copy(s.trial.begin(), s.trial.end(), W.begin() + (size_t)nc * P);
            cmap[nc++] = k;
        }
        if (nc == 0) break;
        F2VC(logreg_pass(c, pairs, m, feature, classes, cmap.data(), nc, W.data(), lambda, loss.data(), grad.data(), &seconds));
        for (uint32_t i = 0; i < nc; i++) {
            LbfgsClass &s = cls[cmap[i]];
            s.evaluations++;
            if (loss[i] <= s.f + 1e-4 * s.t * s.gp) {  // (a NaN loss is no descent)
                std::vector<double> sv(P), yv(P);
                for (uint32_t j = 0; j < P; j++) {
                    sv[j] = s.trial[j] - s.w[j];
                    yv[j] = grad[(size_t)i * P + j] - s.g[j];
                }
                const double sy = lr_dot(sv, yv);
                if (sy > 0.0) {
                    if (s.S.size() == 10) {
                        s.S.erase(s.S.begin());
                        s.Y.erase(s.Y.begin());
                        s.rho.erase(s.rho.begin());
                    }
                    s.S.push_back(sv);
                    s.Y.push_back(yv);
                    s.rho.push_back(1.0 / sy);
                }
                s.w = s.trial;
                s.g.assign(grad.begin() + (size_t)i * P, grad.begin() + (size_t)(i + 1) * P);
                s.f = loss[i];
                s.iterations++;
                s.searching = false;
                s.gnorm = lr_norm_inf(s.g);
                s.converged = s.gnorm <= stop;
                if (s.converged || s.iterations >= max_iter) s.active = false;
            } else if (++s.halvings > 40) {
                s.active = false;  // the line search failed: the class stays at its last accepted point
            } else {
                s.t *= 0.5;
            }
        }
    }
    F2VC(check_kernel_err(c, "f2v_logreg_fit"));
    for (uint32_t k = 0; k < classes; k++) {
        const LbfgsClass &s = cls[k];
        std::copy(s.w.begin(), s.w.end(), weights_out + (size_t)k * P);
        f2v_logreg_t info{};
        info.loss = s.f;
        info.gnorm_inf = s.gnorm;
        info.seconds = seconds;
        info.iterations = s.iterations;
        info.evaluations = s.evaluations;
        info.converged = s.converged;
        info_out[k] = info;
    }
    return F2V_OK;
}

int f2v_logreg_decision(f2v_handle c, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const double *weights, uint32_t classes,
                        double *z_out, double *seconds_out) {
    if (!c || !a_ids || !weights || !z_out) return fail(F2V_EINVAL, "f2v_logreg_decision: null argument");
    F2VC(logreg_enter(c, "f2v_logreg_decision", a_ids, b_ids, m, feature, nullptr, classes));
    f2v_ctx::Logreg &w = c->lr;
    F2VC(w.d_z.reserve(c, (size_t)std::min(m, kLrDecisionChunk) * classes, "logistic-regression"));
    HIPC(hipMemcpyAsync(w.d_W, weights, (size_t)classes * (c->D + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double seconds = 0.0;
    for (uint32_t lo = 0; lo < m; lo += kLrDecisionChunk) {
        const uint32_t cnt = std::min(m - lo, kLrDecisionChunk);
        LrArgs a = logreg_args(c, b_ids != nullptr, cnt, feature, classes, classes);
        a.a += lo;
        a.b += lo;
        a.out = w.d_z;
        F2VC(w.timer.start(c->stream));
        F2VC(launch_logreg(c, a, false));
        F2VC(w.timer.stop(c->stream));
        HIPC(hipMemcpyAsync(z_out + (size_t)lo * classes, w.d_z, (size_t)cnt * classes * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        F2VC(w.timer.seconds(&seconds));
    }
    F2VC(check_kernel_err(c, "f2v_logreg_decision"));
    if (seconds_out) *seconds_out = seconds;
    return F2V_OK;
}

int f2v_nearest_rows(f2v_handle c, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint32_t flags, uint32_t *ids_out,
                     float *scores_out, double *seconds_out) {
    if (!c || (nq && (!query_ids || !ids_out))) return fail(F2V_EINVAL, "f2v_nearest_rows: null argument");
    for (uint32_t i = 0; i < nq; i++)
        if (query_ids[i] >= c->n) return fail(F2V_EINVAL, "f2v_nearest_rows: query_ids[%u] = %u is not a vertex", i, query_ids[i]);
    int rc = nearest_enter(c, "f2v_nearest_rows", nq, k, metric, flags, (flags & F2V_NEAREST_EXCLUDE_NEIGHBOURS) != 0);
    if (rc == 1) {
        if (seconds_out) *seconds_out = 0.0;
        return F2V_OK;
    }
    if (rc != F2V_OK) return rc;
    return nearest_run(c, query_ids, false, nullptr, nq, k, metric, flags, ids_out, scores_out, nullptr, seconds_out);
}

int f2v_nearest_vectors(f2v_handle c, const float *queries, uint32_t nq, uint32_t k, int metric, uint32_t *ids_out, float *scores_out,
                        double *seconds_out) {
    if (!c || (nq && (!queries || !ids_out))) return fail(F2V_EINVAL, "f2v_nearest_vectors: null argument");
    int rc = nearest_enter(c, "f2v_nearest_vectors", nq, k, metric, 0, false);
    if (rc == 1) {
        if (seconds_out) *seconds_out = 0.0;
        return F2V_OK;
    }
    if (rc != F2V_OK) return rc;
    return nearest_run(c, nullptr, false, queries, nq, k, metric, 0, ids_out, scores_out, nullptr, seconds_out);
}

int f2v_neighbour_recall(f2v_handle c, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint64_t *hits_out,
                         uint64_t *possible_out, double *seconds_out) {
    if (!c || !hits_out || !possible_out) return fail(F2V_EINVAL, "f2v_neighbour_recall: null argument");
    if (!query_ids) nq = c->n;
    for (uint32_t i = 0; query_ids && i < nq; i++)
        if (query_ids[i] >= c->n) return fail(F2V_EINVAL, "f2v_neighbour_recall: query_ids[%u] = %u is not a vertex", i, query_ids[i]);
    int rc = nearest_enter(c, "f2v_neighbour_recall", nq, k, metric, 0, true);
    if (rc == 1) {  // no queries: 0 of 0
        *hits_out = *possible_out = 0;
        if (seconds_out) *seconds_out = 0.0;
        return F2V_OK;
    }
    if (rc != F2V_OK) return rc;
    uint64_t counts[2] = {0, 0};
    rc = nearest_run(c, query_ids, !query_ids, nullptr, nq, k, metric, F2V_NEAREST_EXCLUDE_SELF, nullptr, nullptr, counts, seconds_out);
    if (rc != F2V_OK) return rc;
    *hits_out = counts[0];
    *possible_out = counts[1];
    return F2V_OK;
}

int f2v_index_build(f2v_handle c, uint32_t lists, uint32_t max_iters, uint64_t seed, const float *init_centroids, f2v_index_t *info_out) {
    if (!c) return fail(F2V_EINVAL, "f2v_index_build: null argument");
    if (lists == 0 || lists > F2V_INDEX_MAX_LISTS || lists > c->n)
        return fail(F2V_EINVAL, "f2v_index_build: lists = %u is outside 1..min(%d, n = %u)", lists, F2V_INDEX_MAX_LISTS, c->n);
    std::vector<uint32_t> labels(c->n);
    std::vector<float> centroids((size_t)lists * c->D);
    f2v_kmeans_t km{};
    F2VC(f2v_kmeans(c, lists, max_iters, 1, seed, init_centroids, labels.data(), centroids.data(), nullptr, &km));
    return index_install(c, "f2v_index_build", labels.data(), centroids.data(), lists, &km, info_out);
}

int f2v_index_build_given(f2v_handle c, const uint32_t *labels, const float *centroids, uint32_t lists, f2v_index_t *info_out) {
    if (!c || !labels || !centroids) return fail(F2V_EINVAL, "f2v_index_build_given: null argument");
    if (lists == 0 || lists > F2V_INDEX_MAX_LISTS || lists > c->n)
        return fail(F2V_EINVAL, "f2v_index_build_given: lists = %u is outside 1..min(%d, n = %u)", lists, F2V_INDEX_MAX_LISTS, c->n);
    if (c->n >= 0xFFFFFFFFu - 256u) return fail(F2V_EINVAL, "f2v_index_build_given: too many vertices for 32-bit row blocks");
    return index_install(c, "f2v_index_build_given", labels, centroids, lists, nullptr, info_out);
}

int f2v_index_get(f2v_handle c, uint32_t *labels_out, float *centroids_out, uint64_t *counts_out, f2v_index_t *info_out) {
    if (!c) return fail(F2V_EINVAL, "f2v_index_get: null argument");
    f2v_ctx::Index &w = c->ix;
    if (!w.built) return fail(F2V_ESTATE, "f2v_index_get: the handle has no index: build one first");
    HIPC(hipSetDevice(c->device));
    if (labels_out) HIPC(hipMemcpyAsync(labels_out, w.d_labels, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (centroids_out) HIPC(hipMemcpyAsync(centroids_out, w.d_C, (size_t)w.info.lists * c->D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (uint32_t l = 0; counts_out && l < w.info.lists; l++) counts_out[l] = w.offsets[l + 1] - w.offsets[l];
    if (info_out) *info_out = w.info;
    return F2V_OK;
}

int f2v_index_drop(f2v_handle c) {
    if (!c) return fail(F2V_EINVAL, "f2v_index_drop: null argument");
    (void)hipSetDevice(c->device);
    index_drop(c);
    return F2V_OK;
}

int f2v_index_search_rows(f2v_handle c, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint32_t flags, uint32_t nprobe,
                          uint32_t *ids_out, float *scores_out, uint32_t *probes_out, f2v_index_search_t *info_out) {
    if (!c || (nq && (!query_ids || !ids_out))) return fail(F2V_EINVAL, "f2v_index_search_rows: null argument");
    for (uint32_t i = 0; i < nq; i++)
        if (query_ids[i] >= c->n) return fail(F2V_EINVAL, "f2v_index_search_rows: query_ids[%u] = %u is not a vertex", i, query_ids[i]);
    const int rc = index_enter(c, "f2v_index_search_rows", nq, k, metric, flags, nprobe, info_out);
    if (rc != F2V_OK) return rc == 1 ? F2V_OK : rc;
    return index_search(c, "f2v_index_search_rows", query_ids, nullptr, nq, k, metric, flags, nprobe, ids_out, scores_out, probes_out, info_out);
}

int f2v_index_search_vectors(f2v_handle c, const float *queries, uint32_t nq, uint32_t k, int metric, uint32_t nprobe, uint32_t *ids_out,
                             float *scores_out, uint32_t *probes_out, f2v_index_search_t *info_out) {
    if (!c || (nq && (!queries || !ids_out))) return fail(F2V_EINVAL, "f2v_index_search_vectors: null argument");
    const int rc = index_enter(c, "f2v_index_search_vectors", nq, k, metric, 0, nprobe, info_out);
    if (rc != F2V_OK) return rc == 1 ? F2V_OK : rc;
    return index_search(c, "f2v_index_search_vectors", nullptr, queries, nq, k, metric, 0, nprobe, ids_out, scores_out, probes_out, info_out);
}

int f2v_push_export(f2v_handle c, void *handles_out) {
    if (!c || !handles_out) return fail(F2V_EINVAL, "f2v_push_export: null argument");
    HIPC(hipSetDevice(c->device));
    if (c->push.attached) return fail(F2V_ESTATE, "f2v_push_export: detach first");
    int rc = flush_pending(c);
    if (rc != F2V_OK) return rc;
    HIPC(hipStreamSynchronize(c->stream));
    // fresh, zeroed flags for every attachment: no peer can write them before it has seen this export
    c->push.flags.release();
    F2VC(c->push.flags.reserve(4096 / sizeof(unsigned long long), "push flags", true));
    HIPC(hipMemset(c->push.flags, 0, 4096));
    F2VC(c->push.d_err.reserve(16, "push error words"));
    HIPC(hipMemset(c->push.d_err, 0, 64));
    HIPC(hipDeviceSynchronize());
    c->push.seq = 0;
    c->push.round = 0;
    PushExport e{};
    const size_t matrix_bytes = ((size_t)c->n + kPadRows) * c->D * sizeof(float);
    // What HIP IPC can map.  Evidence (tools/ipc_probe.py, ROCm 7.2, dmabuf IPC, HSA_ENABLE_IPC_MODE_LEGACY=0): an allocation one
    // row below 2^31 bytes attaches in a millisecond, one row above 2^31 bytes never returns from hipIpcOpenMemHandle -- the
    // step is at exactly 2^31 BYTES OF ALLOCATION SIZE, whatever the row count, padding or matrix contents, and the 4-KiB
    // fine-grained flag array and the landing buffers (<= 1 GiB) always attach: a signed 32-bit size on the import path of the
    // IPC handle, not a property of peer access or of lazy enabling (the same flag maps the small allocations).  So the
    // threshold IS that number; tests/test_gpu_large.py attaches one matrix just below it directly and one just above it
    // through the landing buffer.  Only ever observed with both processes on one GPU (no multi-GPU box was available).
    c->push.landing = c->push.force_landing || matrix_bytes >= kIpcMaxBytes;
    if (c->push.landing) {
        // two halves of at most 512 MiB; room for the self-test's `world` pattern rows in any case
        const size_t per_row = (size_t)c->D * sizeof(float);
        c->push.landing_cap = (uint32_t)std::max<size_t>(std::min<size_t>(((size_t)512 << 20) / per_row, (size_t)c->n + kPadRows), 64);
        c->push.landing_buf.release();
        F2VC(c->push.landing_buf.reserve(2 * (size_t)c->push.landing_cap * c->D, "landing buffer"));
        HIPC(hipIpcGetMemHandle(&e.x[0], c->push.landing_buf));
    } else {
        for (int k = 0; k < 2; k++) HIPC(hipIpcGetMemHandle(&e.x[k], c->d_X[k]));
    }
    HIPC(hipIpcGetMemHandle(&e.flags, c->push.flags));
    e.magic = kPushMagic;
    e.n = c->n;
    e.D = c->D;
    e.cur = (uint32_t)c->cur;
    e.landing = c->push.landing ? 1u : 0u;
    e.landing_cap = c->push.landing_cap;
    memset(e.bus_id, 0, sizeof e.bus_id);
    {
        char bus[64] = {};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, c->device) == hipSuccess) strncpy(e.bus_id, bus, sizeof e.bus_id - 1);
    }
    e.caps = c->xcc_round_robin ? 1u : 0u;
    memcpy(handles_out, &e, sizeof e);
    c->push.exported = true;
    return F2V_OK;
}

int f2v_push_attach(f2v_handle c, uint32_t rank, uint32_t world, const void *all_handles) {
    if (!c || !all_handles) return fail(F2V_EINVAL, "f2v_push_attach: null argument");
    if (world == 0 || world > (uint32_t)kMaxRanks || rank >= world) return fail(F2V_EINVAL, "f2v_push_attach: rank %u of %u (at most %d ranks)", rank, world, kMaxRanks);
    if (!c->push.exported) return fail(F2V_ESTATE, "f2v_push_attach: f2v_push_export first");
    if (c->push.attached) return fail(F2V_ESTATE, "f2v_push_attach: already attached");
    HIPC(hipSetDevice(c->device));
    const PushExport *all = static_cast<const PushExport *>(all_handles);
    for (uint32_t r = 0; r < world; r++) {
        PushExport e;
        memcpy(&e, all + r, sizeof e);
        if (e.magic != kPushMagic) return fail(F2V_EINVAL, "f2v_push_attach: export of rank %u is not an export", r);
        if (e.n != c->n || e.D != c->D || e.cur != (uint32_t)c->cur)
            return fail(F2V_ESTATE, "f2v_push_attach: rank %u holds a different engine state (n %u dim %u matrix %u; here %u %u %d)", r, e.n, e.D, e.cur, c->n, c->D, c->cur);
        if ((e.landing != 0) != c->push.landing || (c->push.landing && e.landing_cap != c->push.landing_cap))
            return fail(F2V_ESTATE, "f2v_push_attach: rank %u exchanges through %s, this rank through %s (\"push_landing\" must agree)", r,
                        e.landing ? "a landing buffer" : "mapped matrices", c->push.landing ? "a landing buffer" : "mapped matrices");
    }
    {
        PushExport me;
        memcpy(&me, all + rank, sizeof me);
        bool shared = false;
        for (uint32_t r = 0; r < world; r++) {
            PushExport e;
            memcpy(&e, all + r, sizeof e);
            if (r != rank && (me.bus_id[0] == 0 || !memcmp(e.bus_id, me.bus_id, sizeof me.bus_id))) shared = true;
        }
        if (shared != c->shared_card) {  // placement of the hub pieces depends on it
            c->shared_card = shared;
            drop_plans(c);
        }
        // what every rank must decide alike ("replicate_small"): do any two ranks share a card, can every rank chain
        c->push.any_shared = false;
        c->push.all_chain = true;
        for (uint32_t r = 0; r < world; r++) {
            PushExport e;
            memcpy(&e, all + r, sizeof e);
            if (!(e.caps & 1u)) c->push.all_chain = false;
            for (uint32_t q = r + 1; q < world; q++) {
                PushExport f;
                memcpy(&f, all + q, sizeof f);
                if (e.bus_id[0] == 0 || !memcmp(e.bus_id, f.bus_id, sizeof e.bus_id)) c->push.any_shared = true;
            }
        }
    }
    c->push.rank = rank;
    c->push.world = world;
    c->push.attached = true;  // from here on push_detach unmaps whatever got mapped
    for (uint32_t r = 0; r < world; r++) {
        if (r == rank) {
            for (int k = 0; k < 2; k++) c->push.peer_X[k][r] = c->d_X[k];
            c->push.peer_flags[r] = c->push.flags;
            c->push.peer_landing[r] = c->push.landing_buf;
            continue;
        }
        PushExport e;
        memcpy(&e, all + r, sizeof e);
        if (c->push.landing) {
            hipError_t he = hipIpcOpenMemHandle((void **)&c->push.peer_landing[r], e.x[0], hipIpcMemLazyEnablePeerAccess);
            if (he != hipSuccess) {
                c->push.peer_landing[r] = nullptr;
                (void)push_detach(c);
                return fail(F2V_ENODEV, "f2v_push_attach: cannot map the landing buffer of rank %u: %s", r, hipGetErrorString(he));
            }
        }
        for (int k = 0; k < 2 && !c->push.landing; k++) {
            hipError_t he = hipIpcOpenMemHandle((void **)&c->push.peer_X[k][r], e.x[k], hipIpcMemLazyEnablePeerAccess);
            if (he != hipSuccess) {
                c->push.peer_X[k][r] = nullptr;
                (void)push_detach(c);
                return fail(F2V_ENODEV, "f2v_push_attach: cannot map the matrix of rank %u: %s", r, hipGetErrorString(he));
            }
        }
        hipError_t he = hipIpcOpenMemHandle((void **)&c->push.peer_flags[r], e.flags, hipIpcMemLazyEnablePeerAccess);
        if (he != hipSuccess) {
            c->push.peer_flags[r] = nullptr;
            (void)push_detach(c);
            return fail(F2V_ENODEV, "f2v_push_attach: cannot map the flags of rank %u: %s", r, hipGetErrorString(he));
        }
    }
    c->push.mask_batch = 0;  // masks depend on (rank, world)
    c->push.exported = false;
    return F2V_OK;
}

#ifdef F2V_TEST_HOOKS
int f2v_test_withhold_flag(f2v_handle c, uint32_t slot) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    c->hooks.withhold_slot = slot;
    return F2V_OK;
}

int f2v_test_withhold_row(f2v_handle c, uint32_t row) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    c->hooks.withhold_row = row;
    return F2V_OK;
}

int f2v_test_chain_nowait(f2v_handle c, int on) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    c->hooks.chain_mode = (uint32_t)on;
    return F2V_OK;
}

int f2v_test_interaction_stub(f2v_handle c, uint32_t mode) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    c->hooks.stub = mode & 3u;
    return F2V_OK;
}

// Host-only check of the wide form's launch plans (no device is touched): builds the programs of one epoch for a graph and a
// set of tunables exactly as f2v_train would and verifies what the kernel relies on --
//   * every row is finished exactly once (by a whole-row item, a row job, or the root of a combine tree), every neighbour of a
//     split row belongs to exactly one piece, first / last pieces are flagged as such;
//   * a workgroup's items fill whole rounds, the items of a round agree on whether it ends a phase, piece slots and job ranges
//     stay inside the LDS slot space, passes hold at most 8 jobs, a job adds consecutive pieces of ONE row in neighbour order;
//   * WAITS ONLY POINT BACKWARDS: a helper's group sum is produced by a workgroup with a smaller index than the finisher that
//     imports it, every sum a combine-tree node adds by a smaller index than the node's, minibatches appear in order.
// stats_out[0..6]: workgroups, helpers, finishers, packed workgroups, node workgroups, partial-sum slots, a checksum of the plan arrays.
int f2v_test_wide_plan_check(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint64_t nnz, uint32_t dim, uint32_t batch, int walk,
                             const char *const *names, const int64_t *values, uint32_t n_params, uint64_t *stats_out) {
    if (!rowptr || (!colids && nnz) || n < 2 || dim == 0 || batch == 0) return fail(F2V_EINVAL, "f2v_test_wide_plan_check: bad argument");
    f2v_ctx ctx;
    f2v_ctx *c = &ctx;
    unsigned plan_threads = 0;
    c->n = n; c->nnz = nnz; c->D = dim;
    c->rowptr.assign(rowptr, rowptr + n + 1);
    c->colids.assign(colids, colids + nnz);
    c->chunk = auto_chunk(c, batch);
    // overrides go into the handle's fields as f2v_set_param would store them (no device is there to quiesce); only what the planner reads
    static const char *const planner_reads[] = {"hub_chunk", "hub_fanin", "class_cut", "wide_phases", "wide_rounds", "wide_span", "wide_finish", "wide_order", "wide_rows", "wide_min_width"};
    for (uint32_t k = 0; k < n_params; k++) {
        const char *nm = names[k];
        if (!strcmp(nm, "plan_threads")) plan_threads = (unsigned)values[k];  // build the epoch's plans on this many host threads (wide_plans_for_epoch)
        else if (std::any_of(std::begin(planner_reads), std::end(planner_reads), [&](const char *r) { return !strcmp(r, nm); })) find_param(nm)->put(c, values[k]);
        else return fail(F2V_EINVAL, "f2v_test_wide_plan_check: unknown parameter '%s'", nm);
    }
    if (!wide_usable(c) || subwave_width(c) == 0) return fail(F2V_EINVAL, "f2v_test_wide_plan_check: the wide form does not run this shape");
    const uint32_t nb = (uint32_t)(((uint64_t)n + batch - 1) / batch), K = chain_len(c, batch, true);
    const uint32_t width = wide_width(c, batch), ipb = wide_items_per_block(width), pslots = std::max<uint32_t>(ipb, 32u), F = c->fanin;
    std::vector<uint32_t> finished(n, 0), covered(nnz, 0);
    uint64_t st[7] = {};
    if (plan_threads) wide_plans_for_epoch(c, nb, K, batch, walk != 0, plan_threads);
#define F2V_PLAN_FAIL(...) return fail(F2V_ESTATE, "f2v_test_wide_plan_check: " __VA_ARGS__)
    for (uint32_t b0 = 0; b0 < nb; b0 += K) {
        const WidePlan p = wide_plan_for(c, b0, std::min(K, nb - b0), batch, walk != 0);
        if (c->plan_overflow) F2V_PLAN_FAIL("slot overflow");
        st[0] += p.n_wgs; st[1] += p.n_helpers; st[2] += p.n_finishers; st[3] += p.n_packed; st[4] += p.n_node_wgs; st[5] = std::max<uint64_t>(st[5], p.n_slots);
        // partial-sum slot -> who announces it: 4 * workgroup + wavefront for a tree node (one node per wavefront: a node may wait for an
        // earlier wavefront of its own workgroup -- they are resident together), 4 * workgroup + 3 for a job (its consumer must be a LATER workgroup)
        std::vector<int64_t> producer(p.n_slots + 1, -1);
        uint32_t last_lo = 0;
        // pass 1: who produces which slot
        for (uint32_t wgi = 0; wgi < p.n_wgs; wgi++) {
            const WideDesc &d = c->plan_wide.h[p.wg_off + wgi];
            if (d.kind == 0) {
                for (uint32_t j = 0; j < d.d; j++) {
                    const WJob &jb = c->plan_jobs.h[p.job_off + d.c + j];
                    if (jb.kind == kJobPart) {
                        if (jb.dst >= p.n_slots || producer[jb.dst] != -1) F2V_PLAN_FAIL("partial-sum slot %u produced twice or out of range", jb.dst);
                        producer[jb.dst] = 4 * (int64_t)wgi + 3;
                    }
                }
            } else {
                for (uint32_t w = 0; w < 4 && d.c * 4 + w < d.b; w++) {
                    const FinItem &h = c->plan_hubs.h[p.fin_off + d.a + d.c * 4 + w];
                    if (h.n == 0) continue;
                    if (h.out != kFinToStage) {
                        if (h.out >= p.n_slots || producer[h.out] != -1) F2V_PLAN_FAIL("tree node output slot %u produced twice or out of range", h.out);
                        producer[h.out] = 4 * (int64_t)wgi + w;
                    }
                }
            }
        }
        // pass 2: every workgroup
        for (uint32_t wgi = 0; wgi < p.n_wgs; wgi++) {
            const WideDesc &d = c->plan_wide.h[p.wg_off + wgi];
            if (d.lo < last_lo || d.lo < p.lo || d.lo >= p.hi) F2V_PLAN_FAIL("workgroup %u: minibatch at row %u out of order", wgi, d.lo);
            last_lo = d.lo;
            const uint32_t mb_hi = (uint32_t)std::min<uint64_t>((uint64_t)d.lo + batch, n);
            if (d.kind == 1) {
                for (uint32_t w = 0; w < 4 && d.c * 4 + w < d.b; w++) {
                    const FinItem &h = c->plan_hubs.h[p.fin_off + d.a + d.c * 4 + w];
                    if (h.n == 0) continue;
                    for (uint32_t k = 0; k < h.n; k++)
                        if (h.in_slot + k >= p.n_slots || producer[h.in_slot + k] < 0 || producer[h.in_slot + k] >= 4 * (int64_t)wgi + w)
                            F2V_PLAN_FAIL("tree node of row %u (workgroup %u) adds slot %u whose producer is not an earlier workgroup (or an earlier wavefront of its own)", h.row, wgi, h.in_slot + k);
                    if (h.out == kFinToStage) {
                        if (h.row < d.lo || h.row >= mb_hi) F2V_PLAN_FAIL("tree root of row %u outside its minibatch", h.row);
                        finished[h.row]++;
                    }
                }
                continue;
            }
            const Item *items = c->plan_items.h.data() + p.item_off + d.a;
            const WJob *jobs = c->plan_jobs.h.data() + p.job_off + d.c;
            if (d.b == 0) F2V_PLAN_FAIL("workgroup %u has no round", wgi);
            // phases: rounds up to a round whose items carry kItemPhaseEnd
            std::vector<std::vector<const Item *>> phase_items(1);
            for (uint32_t r = 0; r < d.b; r++) {
                const bool end = (items[(size_t)r * ipb].flags & kItemPhaseEnd) != 0;
                for (uint32_t q = 0; q < ipb; q++) {
                    const Item &it = items[(size_t)r * ipb + q];
                    if (((it.flags & kItemPhaseEnd) != 0) != end) F2V_PLAN_FAIL("workgroup %u round %u: items disagree about the end of the phase", wgi, r);
                    if (it.flags & kItemIdle) continue;
                    if (it.row < d.lo || it.row >= mb_hi) F2V_PLAN_FAIL("workgroup %u: row %u outside its minibatch [%u,%u)", wgi, it.row, d.lo, mb_hi);
                    if (!walk) {
                        if (it.nb < rowptr[it.row] || it.nb + it.cnt > rowptr[it.row + 1]) F2V_PLAN_FAIL("row %u: piece outside the row's neighbours", it.row);
                        for (uint32_t e = 0; e < it.cnt; e++) covered[it.nb + e]++;
                        if (((it.flags & kItemFirst) != 0) != (it.nb == rowptr[it.row]) || ((it.flags & kItemLast) != 0) != (it.nb + it.cnt == rowptr[it.row + 1]))
                            F2V_PLAN_FAIL("row %u: first / last flags of a piece are wrong", it.row);
                    }
                    if (it.flags & kItemDirect) finished[it.row]++;
                    else if ((it.flags & kItemPieceSlot) >= pslots) F2V_PLAN_FAIL("row %u: piece slot out of range", it.row);
                    phase_items.back().push_back(&it);
                }
                if (end && r + 1 < d.b) phase_items.emplace_back();
                if (!end && r + 1 == d.b) F2V_PLAN_FAIL("workgroup %u: the last round does not end a phase", wgi);
            }
            uint32_t last_phase = 0;
            bool before_ok = true;
            for (uint32_t j = 0; j < d.d; j++) {
                const WJob &jb = jobs[j];
                if (jb.pass_len == 0 || jb.pass_len > 8) F2V_PLAN_FAIL("workgroup %u: a pass of %u jobs", wgi, jb.pass_len);
                if (jb.phase == kJobBefore) { if (!before_ok) F2V_PLAN_FAIL("workgroup %u: a before-the-first-round job behind a phase job", wgi); }
                else {
                    before_ok = false;
                    if (jb.phase < last_phase || jb.phase >= phase_items.size()) F2V_PLAN_FAIL("workgroup %u: job phases out of order", wgi);
                    last_phase = jb.phase;
                }
                if (jb.kind == kJobImport) {
                    if (jb.dst < pslots || jb.dst >= pslots + kWideSumSlots) F2V_PLAN_FAIL("workgroup %u: an import lands outside the sum slots", wgi);
                    if (jb.row >= p.n_slots || producer[jb.row] < 0 || producer[jb.row] >= 4 * (int64_t)wgi)
                        F2V_PLAN_FAIL("workgroup %u imports slot %u whose producer is not an earlier workgroup", wgi, jb.row);
                    continue;
                }
                if (jb.n == 0 || (uint32_t)jb.src + jb.n > pslots + kWideSumSlots) F2V_PLAN_FAIL("workgroup %u: a job's slots are out of range", wgi);
                // piece-slot ranges: consecutive pieces of ONE row, in neighbour order, all in the job's phase
                auto check_pieces = [&](uint32_t first, uint32_t cnt, uint32_t row) -> bool {
                    if (first + cnt > pslots || jb.phase == kJobBefore) return false;
                    uint32_t next_nb = 0;
                    for (uint32_t k = 0; k < cnt; k++) {
                        const Item *hit = nullptr;
                        for (const Item *it : phase_items[jb.phase])
                            if (!(it->flags & kItemDirect) && (it->flags & kItemPieceSlot) == first + k) { if (hit) return false; hit = it; }
                        if (!hit || hit->row != row || (k && hit->nb != next_nb)) return false;
                        next_nb = hit->nb + hit->cnt;
                    }
                    return true;
                };
                if (jb.n2 != 0) {
                    if (jb.dst2 < jb.src || jb.dst2 >= (uint32_t)jb.src + jb.n || jb.pass_len != 1) F2V_PLAN_FAIL("workgroup %u: a fused job's first sum does not land among its second's slots", wgi);
                    if (!walk && !check_pieces(jb.src2, jb.n2, jb.row)) F2V_PLAN_FAIL("row %u: a fused job's pieces are not consecutive pieces of the row", jb.row);
                }
                if (jb.src < pslots) {
                    if (jb.n > F) F2V_PLAN_FAIL("row %u: a job adds %u pieces, more than the fan-in", jb.row, jb.n);
                    if (!walk && !check_pieces(jb.src, jb.n, jb.row)) F2V_PLAN_FAIL("row %u: a job's pieces are not consecutive pieces of the row", jb.row);
                }
                if (jb.kind == kJobLds && (jb.dst < pslots || jb.dst >= pslots + kWideSumSlots)) F2V_PLAN_FAIL("workgroup %u: a group sum lands outside the sum slots", wgi);
                if (jb.kind == kJobRow) {
                    if (jb.row < d.lo || jb.row >= mb_hi) F2V_PLAN_FAIL("row job of row %u outside its minibatch", jb.row);
                    finished[jb.row]++;
                }
            }
        }
    }
#undef F2V_PLAN_FAIL
    for (uint32_t i = 0; i < n; i++)
        if (finished[i] != 1) return fail(F2V_ESTATE, "f2v_test_wide_plan_check: row %u is finished %u times", i, finished[i]);
    if (!walk)
        for (uint64_t e = 0; e < nnz; e++)
            if (covered[e] != 1) return fail(F2V_ESTATE, "f2v_test_wide_plan_check: neighbour %llu is in %u pieces", (unsigned long long)e, covered[e]);
    {   // [6]: a checksum of the resident plan arrays (items, jobs, descriptors, tree nodes): the threaded build leaves the serial build's
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void *p, size_t bytes) {
            const unsigned char *q = static_cast<const unsigned char *>(p);
            for (size_t k = 0; k < bytes; k++) h = (h ^ q[k]) * 1099511628211ull;
        };
        mix(c->plan_items.h.data(), c->plan_items.h.size() * sizeof(Item));
        mix(c->plan_jobs.h.data(), c->plan_jobs.h.size() * sizeof(WJob));
        mix(c->plan_wide.h.data(), c->plan_wide.h.size() * sizeof(WideDesc));
        mix(c->plan_hubs.h.data(), c->plan_hubs.h.size() * sizeof(FinItem));
        st[6] = h;
    }
    if (stats_out) memcpy(stats_out, st, sizeof st);
    return F2V_OK;
}

int f2v_test_stamps(f2v_handle c, int on, unsigned long long *out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    const size_t bytes = 4 * (size_t)c->n * sizeof(unsigned long long);
    if (out) {
        if (!c->hooks.d_stamps) return fail(F2V_ESTATE, "f2v_test_stamps: not switched on");
        HIPC(hipMemcpy(out, c->hooks.d_stamps, bytes, hipMemcpyDeviceToHost));
    }
    if (on) {
        F2VC(c->hooks.d_stamps.reserve(4 * (size_t)c->n, "stamps"));
        HIPC(hipMemsetAsync(c->hooks.d_stamps, 0, bytes, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    } else {
        c->hooks.d_stamps.release();
    }
    return F2V_OK;
}

int f2v_test_push_attach_local(f2v_handle c, uint32_t rank, uint32_t world, const f2v_handle *all) {
    if (!c || !all) return fail(F2V_EINVAL, "f2v_test_push_attach_local: null argument");
    if (world == 0 || world > (uint32_t)kMaxRanks || rank >= world || all[rank] != c) return fail(F2V_EINVAL, "f2v_test_push_attach_local: rank %u of %u", rank, world);
    if (!c->push.exported) return fail(F2V_ESTATE, "f2v_test_push_attach_local: f2v_push_export first (it creates the flags)");
    if (c->push.attached) return fail(F2V_ESTATE, "f2v_test_push_attach_local: already attached");
    for (uint32_t r = 0; r < world; r++) {
        if (!all[r] || !all[r]->push.flags || all[r]->n != c->n || all[r]->D != c->D || all[r]->cur != c->cur || all[r]->device != c->device)
            return fail(F2V_ESTATE, "f2v_test_push_attach_local: peer %u is not an exported engine of the same shape on the same device", r);
        for (int k = 0; k < 2; k++) c->push.peer_X[k][r] = all[r]->d_X[k];
        c->push.peer_flags[r] = all[r]->push.flags;
        c->push.peer_landing[r] = all[r]->push.landing_buf;
        if (all[r]->push.landing != c->push.landing) return fail(F2V_ESTATE, "f2v_test_push_attach_local: \"push_landing\" must agree");
    }
    if (!c->shared_card && world > 1) { c->shared_card = true; drop_plans(c); }
    c->push.rank = rank;
    c->push.world = world;
    c->push.attached = c->push.local = true;
    c->push.mask_batch = 0;
    c->push.exported = false;
    return F2V_OK;
}

#endif  // F2V_TEST_HOOKS

int f2v_push_detach(f2v_handle c) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    HIPC(hipSetDevice(c->device));
    return push_detach(c);
}

int f2v_push_selftest(f2v_handle c) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (!c->push.attached) return fail(F2V_ESTATE, "f2v_push_selftest: f2v_push_attach first");
    HIPC(hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc != F2V_OK) return rc;
    const uint32_t W = c->push.world, me = c->push.rank, D = c->D;
    const int which = c->cur ^ 1;  // the slack rows behind row N of the matrix no epoch is reading
    // a pattern nobody could hold by accident: depends on the rank and on how many barriers have passed (the same
    // number on every rank)
    const unsigned long long nonce = c->push.seq;
    auto value = [&](uint32_t r, uint32_t d) { return (float)(1 + r) * 1000.0f + (float)(nonce % 977) + (float)d / 1024.0f; };
    std::vector<float> row(D);
    for (uint32_t d = 0; d < D; d++) row[d] = value(me, d);
    HIPC(hipMemcpyAsync(c->d_X[which] + (size_t)(c->n + me) * D, row.data(), D * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if ((rc = launch_barrier(c)) != F2V_OK) return rc;  // nobody pushes before everybody has laid its pattern down
    // as a "minibatch" [n, n+W) of which this rank computed row n+me: lands in the peers' slack rows, or in slot `me` of
    // their landing buffers, from where the exchange's second half moves it to the slack rows
    if ((rc = launch_push(c, which, nullptr, c->n, c->n + me, c->n + me + 1)) != F2V_OK) return rc;
    if ((rc = finish_exchange(c, which, nullptr, c->n, c->n + W, c->n + me, c->n + me + 1)) != F2V_OK) return rc;
    HIPC(hipStreamSynchronize(c->stream));
    if ((rc = check_push_err(c, "f2v_push_selftest")) != F2V_OK) return rc;
    std::vector<float> got((size_t)W * D);
    HIPC(hipMemcpy(got.data(), c->d_X[which] + (size_t)c->n * D, got.size() * sizeof(float), hipMemcpyDeviceToHost));
    bool ok = true;
    for (uint32_t r = 0; r < W && ok; r++)
        for (uint32_t d = 0; d < D; d++)
            if (got[(size_t)r * D + d] != value(r, d)) { ok = false; break; }
    if ((rc = launch_barrier(c)) != F2V_OK) return rc;  // nobody reuses the slack rows before everybody has checked
    HIPC(hipStreamSynchronize(c->stream));
    if ((rc = check_push_err(c, "f2v_push_selftest")) != F2V_OK) return rc;
    if (!ok) return fail(F2V_ENODEV, "f2v_push_selftest: a peer's row did not arrive intact");
    return F2V_OK;
}

int f2v_push_stats(f2v_handle c, uint64_t *rows_pushed_out, uint64_t *rows_allgather_out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    if (rows_pushed_out) *rows_pushed_out = c->push.rows_pushed;
    if (rows_allgather_out) *rows_allgather_out = c->push.rows_allgather;
    return F2V_OK;
}

#ifdef F2V_TEST_HOOKS
// PMC calibration hook: gathers `rows` distinct rows of 128 floats (a random permutation, so every
// 512-byte row is fetched exactly once) with the step kernel's access pattern; `reps` launches.
// Known HBM read volume per launch: rows * 512 bytes (+ 4 bytes per row of ids).
int f2v_test_gather_calibration(int device, uint32_t rows, uint32_t reps) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(F2V_ENODEV, "no HIP device visible");
    if (rows < 4) return fail(F2V_EINVAL, "rows");
    HIPC(hipSetDevice(device));
    DevBuf<float> d_t, d_o;
    DevBuf<uint32_t> d_i;
    F2VC(d_t.reserve((size_t)rows * 128, "calibration"));
    F2VC(d_i.reserve(rows, "calibration"));
    F2VC(d_o.reserve(16, "calibration"));
    HIPC(hipMemset(d_t, 0, (size_t)rows * 128 * sizeof(float)));
    std::vector<uint32_t> perm(rows);
    for (uint32_t i = 0; i < rows; i++) perm[i] = i;
    Rand g;
    g.seed(7);
    for (uint32_t i = rows - 1; i > 0; i--) std::swap(perm[i], perm[(uint32_t)(((uint64_t)g.next() * 2147483648ull + (uint64_t)g.next()) % (i + 1))]);
    HIPC(hipMemcpy(d_i, perm.data(), (size_t)rows * sizeof(uint32_t), hipMemcpyHostToDevice));
    for (uint32_t r = 0; r < reps; r++)
        hipLaunchKernelGGL((gather_calibration_kernel<2>), dim3(4096), dim3(256), 0, 0, d_t, d_i, rows, d_o);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    return F2V_OK;
}

// Per-XCD timing of the launches that follow (one launch per minibatch): on = 1 allocates / clears the 32 words (StepArgs::xcd_times), `out`
// (32 words, may be null) receives what has been recorded since; on = 0 frees them.
int f2v_test_xcd_times(f2v_handle c, int on, unsigned long long *out) {
    if (!c) return fail(F2V_EINVAL, "null handle");
    HIPC(hipSetDevice(c->device));
    HIPC(hipStreamSynchronize(c->stream));
    if (out && c->hooks.d_xcd) HIPC(hipMemcpy(out, c->hooks.d_xcd, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (on) {
        F2VC(c->hooks.d_xcd.reserve(32, "XCD times"));
        unsigned long long init[32];
        for (int k = 0; k < 32; k++) init[k] = (k >= 8 && k < 16) ? ~0ull : 0ull;
        HIPC(hipMemcpy(c->hooks.d_xcd, init, sizeof init, hipMemcpyHostToDevice));
    } else {
        c->hooks.d_xcd.release();
    }
    return F2V_OK;
}

// The memory side of one real launch, alone: the plan of minibatch [row_lo, row_hi) (options 5/6 at D = 128: the headline's layout) replayed by
// plan_gather_kernel -- `reps` launches, the best time in microseconds.  The second matrix is written where mode bit 1 is set: the
// handle's embeddings are garbage afterwards.
int f2v_test_plan_gather(f2v_handle c, uint32_t row_lo, uint32_t row_hi, uint32_t mode, uint32_t reps, double *us_out) {
    if (!c || !us_out || row_lo >= row_hi || row_hi > c->n || reps == 0) return fail(F2V_EINVAL, "f2v_test_plan_gather: bad argument");
    if (subwave_width(c) != 128 || c->D != 128) return fail(F2V_EINVAL, "f2v_test_plan_gather: D = 128 only");
    HIPC(hipSetDevice(c->device));
    int rc = flush_pending(c);
    if (rc != F2V_OK) return rc;
    const Plan plan = plan_for(c, row_lo, row_hi, false);
    if ((rc = upload_plans(c)) != F2V_OK) return rc;
    DevBuf<float> d_o;
    F2VC(d_o.reserve(16, "plan gather"));
    DevTimer t;
    const uint32_t G = 1u << ((mode >> 2) & 3u);  // mode bits 2-3: a wavefront takes 1 / 2 / 4 / 8 consecutive groups of items
    const uint32_t blocks = ((plan.n_items + 16u * 8u * G - 1u) / (16u * 8u * G)) * 8u;  // (plan_gather_kernel: workgroup B takes the plan's workgroups B % 8 + 8 (G (B / 8) + k))
    float best = 1e30f;
    for (uint32_t r = 0; r < reps + 2; r++) {
        F2VC(t.start(c->stream));
#define F2V_PG(GG) hipLaunchKernelGGL((plan_gather_kernel<16, 2, 4, GG>), dim3(blocks), dim3(256), 0, c->stream, c->d_X[c->cur], c->d_X[c->cur ^ 1], c->plan_items.d + plan.item_off, plan.n_items, c->d_colids, mode & 3u, d_o)
        if (G == 1) F2V_PG(1); else if (G == 2) F2V_PG(2); else if (G == 4) F2V_PG(4); else F2V_PG(8);
#undef F2V_PG
        F2VC(t.stop(c->stream));
        HIPC(hipEventSynchronize(t.ev[1]));
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        if (r >= 2 && ms < best) best = ms;
    }
    *us_out = best * 1e3;
    return F2V_OK;
}

#endif  // F2V_TEST_HOOKS

// Stand-alone rehearsal of what f2v_push_attach + the push kernels need from the machine, meant to run in a
// THROW-AWAY process before the real engines exist: allocate `bytes` of device memory and a fine-grained flag array
// on `device`, swap IPC handles with the other ranks through files in `dir`, map theirs, store a word at both ends of
// every peer's buffer and into every peer's flags from a kernel, and check what the peers stored here.  Whatever goes
// wrong -- a mapping call that never returns, a fault on the first remote store -- happens to this process.
int f2v_diag_ipc_preflight(int device, uint32_t rank, uint32_t world, const char *dir, uint64_t bytes, double timeout_s) {
    if (!dir || world == 0 || world > (uint32_t)kMaxRanks || rank >= world || bytes < 4096) return fail(F2V_EINVAL, "f2v_diag_ipc_preflight: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(F2V_ENODEV, "f2v_diag_ipc_preflight: device %d of %d", device, ndev);
    HIPC(hipSetDevice(device));
    DevBuf<uint32_t> data;
    DevBuf<unsigned long long> flags;
    F2VC(data.reserve((bytes + 3) / 4, "preflight"));
    HIPC(hipMemset(data, 0, 4096));
    HIPC(hipMemset((char *)data.p + bytes - 4096, 0, 4096));
    F2VC(flags.reserve(4096 / sizeof(unsigned long long), "preflight flags", true));
    HIPC(hipMemset(flags, 0, 4096));
    HIPC(hipDeviceSynchronize());
    struct Blob { hipIpcMemHandle_t data, flags; } mine, theirs;
    HIPC(hipIpcGetMemHandle(&mine.data, data));
    HIPC(hipIpcGetMemHandle(&mine.flags, flags));
    const auto t0 = std::chrono::steady_clock::now();
    auto late = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s; };
    auto path = [&](const char *what, uint32_t r) { return std::string(dir) + "/" + what + "." + std::to_string(r); };
    auto publish = [&](const char *what, const void *p, size_t len) -> bool {
        const std::string tmp = path(what, rank) + ".tmp";
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f) return false;
        const bool ok = fwrite(p, 1, len, f) == len;
        return (fclose(f) == 0) && ok && rename(tmp.c_str(), path(what, rank).c_str()) == 0;
    };
    auto await = [&](const char *what, uint32_t r, void *p, size_t len) -> bool {
        for (;;) {
            FILE *f = fopen(path(what, r).c_str(), "rb");
            if (f) {
                const size_t got = fread(p, 1, len, f);
                fclose(f);
                if (got == len) return true;
            }
            if (late()) return false;
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
    };
    if (!publish("handles", &mine, sizeof mine)) return fail(F2V_EIO, "f2v_diag_ipc_preflight: cannot write into %s", dir);
    PreflightArgs a{};
    a.self = rank;
    a.world = world;
    a.value = 0xF2F00000u + rank;
    a.last_word = bytes / 4 - 1;
    for (uint32_t r = 0; r < world; r++) {
        if (r == rank) { a.data[r] = data; a.flags[r] = flags; continue; }
        if (!await("handles", r, &theirs, sizeof theirs)) return fail(F2V_ESTATE, "f2v_diag_ipc_preflight: rank %u never published its handles", r);
        HIPC(hipIpcOpenMemHandle((void **)&a.data[r], theirs.data, hipIpcMemLazyEnablePeerAccess));
        HIPC(hipIpcOpenMemHandle((void **)&a.flags[r], theirs.flags, hipIpcMemLazyEnablePeerAccess));
    }
    hipLaunchKernelGGL(preflight_write_kernel, dim3(1), dim3(64), 0, 0, a);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    char one = 1;
    if (!publish("stored", &one, 1)) return fail(F2V_EIO, "f2v_diag_ipc_preflight: cannot write into %s", dir);
    for (uint32_t r = 0; r < world; r++)
        if (r != rank && !await("stored", r, &one, 1)) return fail(F2V_ESTATE, "f2v_diag_ipc_preflight: rank %u never finished its stores", r);
    std::vector<uint32_t> head(world), tail(world);
    std::vector<unsigned long long> fl(world);
    HIPC(hipMemcpy(head.data(), data, world * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(tail.data(), data + a.last_word + 1 - world, world * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(fl.data(), flags, world * 8, hipMemcpyDeviceToHost));
    int bad = 0;
    for (uint32_t r = 0; r < world; r++) {
        const uint32_t want = 0xF2F00000u + r;
        if (head[r] != want || tail[world - 1 - r] != want || fl[r] != want) bad++;
    }
    if (!publish("checked", &one, 1)) return fail(F2V_EIO, "f2v_diag_ipc_preflight: cannot write into %s", dir);
    for (uint32_t r = 0; r < world; r++)  // nobody unmaps or frees while a peer may still be reading
        if (r != rank && !await("checked", r, &one, 1)) break;
    for (uint32_t r = 0; r < world; r++)
        if (r != rank) { (void)hipIpcCloseMemHandle(a.data[r]); (void)hipIpcCloseMemHandle(a.flags[r]); }
    if (bad) return fail(F2V_ENODEV, "f2v_diag_ipc_preflight: %d of %u peers' stores did not arrive intact", bad, world);
    return F2V_OK;
}

// Random-row gather ceiling of this card: every 512-byte row of a `table_bytes` table is fetched exactly once per pass, in
// random order, with the step kernel's access pattern (16 lanes x dwordx4 per row, 4 rows in flight per item); enough
// passes per launch to gather about 2 GiB.  Small tables measure the Infinity Cache / L2, tables far beyond 256 MiB the HBM.
int f2v_diag_gather_rate(int device, uint64_t table_bytes, uint32_t reps, double *gbps_out) {
    if (!gbps_out || table_bytes < (1u << 20) || table_bytes > (64ull << 30) || reps == 0) return fail(F2V_EINVAL, "f2v_diag_gather_rate: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(F2V_ENODEV, "no such HIP device");
    HIPC(hipSetDevice(device));
    const uint32_t rows = (uint32_t)(table_bytes / 512);
    const uint32_t passes = (uint32_t)std::max<uint64_t>(1, (2ull << 30) / ((uint64_t)rows * 512));
    const uint64_t n_ids = (uint64_t)rows * passes;
    if (n_ids > 0xFFFFFFF0ull) return fail(F2V_EINVAL, "f2v_diag_gather_rate: table too large");
    std::vector<uint32_t> ids(n_ids);
    Rand g;
    g.seed(11);
    auto big = [&] { return ((uint64_t)g.next() << 31) | (uint64_t)g.next(); };
    for (uint32_t i = 0; i < rows; i++) ids[i] = i;
    for (uint32_t i = rows - 1; i > 0; i--) std::swap(ids[i], ids[(uint32_t)(big() % (i + 1))]);
    for (uint32_t p = 1; p < passes; p++) {  // later passes: the same permutation under another random rotation and stride
        const uint32_t rot = (uint32_t)(big() % rows);
        for (uint32_t i = 0; i < rows; i++) ids[(size_t)p * rows + i] = ids[(i + rot) % rows] ^ 0u;
    }
    DevBuf<float> d_t, d_o;
    DevBuf<uint32_t> d_i;
    F2VC(d_t.reserve((size_t)rows * 128, "gather rate"));
    F2VC(d_i.reserve(n_ids, "gather rate"));
    F2VC(d_o.reserve(16, "gather rate"));
    HIPC(hipMemset(d_t, 0, (size_t)rows * 512));
    HIPC(hipMemcpy(d_i, ids.data(), n_ids * sizeof(uint32_t), hipMemcpyHostToDevice));
    DevTimer t;
    double best = 0.0;
    for (uint32_t r = 0; r < reps + 2; r++) {
        F2VC(t.start(0));
        hipLaunchKernelGGL((gather_calibration_kernel<2>), dim3(4096), dim3(256), 0, 0, d_t, d_i, (uint32_t)n_ids, d_o);
        F2VC(t.stop(0));
        HIPC(hipEventSynchronize(t.ev[1]));
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        if (r >= 2 && ms > 0.f) best = std::max(best, (double)n_ids * 516.0 / (ms * 1e-3) * 1e-9);
    }
    *gbps_out = best;
    return F2V_OK;
}

// Streaming-copy ceiling of this card: `reps` copies of `bytes` (read + written = 2*bytes each), best rate in GB/s.
int f2v_diag_stream_copy(int device, uint64_t bytes, uint32_t reps, double *gbps_out) {
    if (!gbps_out || bytes < 4096 || reps == 0 || bytes / 16 / 1024 > 0x7FFFFFFFull) return fail(F2V_EINVAL, "f2v_diag_stream_copy: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(F2V_ENODEV, "no such HIP device");
    HIPC(hipSetDevice(device));
    DevBuf<f32x4_copy_t> a, b;
    F2VC(a.reserve((bytes + 15) / 16, "stream copy"));
    F2VC(b.reserve((bytes + 15) / 16, "stream copy"));
    HIPC(hipMemset(a, 1, bytes));
    HIPC(hipDeviceSynchronize());
    DevTimer t;
    double best = 0.0;
    for (uint32_t r = 0; r < reps + 2; r++) {
        F2VC(t.start(0));
        hipLaunchKernelGGL((stream_copy_kernel<4>), dim3((uint32_t)((bytes / 16 + 1023) / 1024)), dim3(256), 0, 0, a, b, (uint64_t)(bytes / 16));
        F2VC(t.stop(0));
        HIPC(hipEventSynchronize(t.ev[1]));
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        if (r >= 2 && ms > 0.f) best = std::max(best, 2.0 * (double)bytes / (ms * 1e-3) * 1e-9);
    }
    *gbps_out = best;
    return F2V_OK;
}

#ifdef F2V_TEST_HOOKS
int f2v_test_wave_reduce(int device, const float *in, uint32_t rows, uint32_t width, float *out) {
    if (!in || !out || width == 0 || width > 512) return fail(F2V_EINVAL, "f2v_test_wave_reduce: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(F2V_ENODEV, "no HIP device visible");
    HIPC(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    F2VC(d_in.reserve((size_t)rows * width, "wave reduce"));
    F2VC(d_out.reserve(rows, "wave reduce"));
    HIPC(hipMemcpy(d_in, in, (size_t)rows * width * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(wave_reduce_test_kernel, dim3((rows + 3) / 4), dim3(256), 0, 0, d_in, rows, width, d_out);
    HIPC(hipGetLastError());
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, d_out, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost));
    return F2V_OK;
}
#endif  // F2V_TEST_HOOKS

}  // extern "C"
