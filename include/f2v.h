/*
 * f2v.h -- C ABI of libf2v, the MI355X (gfx950) Force2Vec embedding engine.
 *
 * Drop-in boundary for the ONE hot path of HipGraph/Force2Vec: the per-minibatch
 * attraction/repulsion force kernels + SGD row update of tForce2Vec / sForce2Vec /
 * rForce2Vec (CLI options 5-7, and 8-11 as their load-balanced equivalents).  The
 * reference has no FFI of its own; each entry point below names the reference interface
 * it replaces (file:line under the reference tree).  Plain pointers and sizes only.
 * Beside training, what the reference judges an embedding by is evaluated on the matrix where it lies, in HBM: the training
 * objective (f2v_objective), nearest rows (f2v_nearest_*), k-means and modularity (f2v_kmeans, f2v_modularity), the
 * logistic-regression scorers of node labels and links (f2v_logreg_*), the separation of a labelling in the embedding space
 * (f2v_silhouette, f2v_davies_bouldin), a two-dimensional picture of the matrix with the score of how faithful it is (f2v_pca,
 * f2v_trustworthiness), and -- the yardstick for the clusters' modularity -- the communities of the graph itself with the agreement of
 * two labellings (f2v_louvain, f2v_partition_agreement); for a held-out link prediction the edge split, the scores and neighbourhood
 * scores of pairs, their ranking, and the filtered rank of every hidden edge among all vertices (f2v_edge_split, f2v_pair_scores,
 * f2v_pair_neighbourhood, f2v_ranking, f2v_pair_ranks).  Each has a definition below that fixes every order of summation, so that its results are
 * functions of its inputs alone.
 *
 * Conventions: every function returns 0 on success and a negative F2V_E* code on failure
 * (f2v_last_error() then holds a message for the calling thread).  The caller owns every
 * host array it passes in (inputs are copied to HBM); the library owns all device state.
 * One handle per host thread; no global mutable state besides the per-thread error text.
 * There is NO CPU fallback: without a usable HIP device f2v_create fails with F2V_ENODEV.
 */
#ifndef F2V_H_
#define F2V_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ABI: libf2v.so is built with -fvisibility=hidden -Wl,-Bsymbolic and exports exactly the functions marked F2V_API
 * (tests/test_host_boundary.py checks `nm -D`).  Nothing else -- no kernel launch stub, no C++ helper -- can be interposed by,
 * or interpose on, another library of the process (two builds of libf2v in one process are two independent engines). */
#ifndef F2V_API
#define F2V_API __attribute__((visibility("default")))
#endif

#define F2V_OK 0
#define F2V_EINVAL (-1)  /* bad argument */
#define F2V_ENODEV (-2)  /* no usable HIP device / HIP runtime error */
#define F2V_ENOMEM (-3)
#define F2V_EIO (-4)
#define F2V_ESTATE (-5)  /* call order violated (e.g. training before init) */

#define F2V_INIT_SYMMETRIC 0 /* randInitF: U[-1,1)  sample/algorithms.cpp:47-53 (options 5,8,11) */
#define F2V_INIT_UNIT 1      /* randInit : U[0,1)   sample/algorithms.cpp:38-45 (options 6,7,9,10) */

typedef struct f2v_ctx *f2v_handle;

F2V_API const char *f2v_last_error(void);
F2V_API const char *f2v_version(void);

/* ---- engine life cycle -----------------------------------------------------------------
 * Replaces `algorithms::algorithms(CSR&, input, outputdir, dim, gamma, batch)`
 * (sample/algorithms.h:60-70): copies the CSR (rowptr u32[n+1], colids u32[nnz], ascending
 * inside each row, duplicates kept -- sample/CSR.h:89-96) to HBM and allocates the N x D
 * fp32 embedding matrix there.  `device` is the HIP device ordinal. */
F2V_API int f2v_create(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint64_t nnz, uint32_t dim, int device,
               f2v_handle *out);
F2V_API int f2v_destroy(f2v_handle h);

/* srand(seed) of Test/Force2Vec.cpp:126; the handle carries the libc rand() stream. */
F2V_API int f2v_srand(f2v_handle h, uint32_t seed);
/* randInitF / randInit (sample/algorithms.cpp:38-53): N*D rand() draws, uploaded to HBM. */
F2V_API int f2v_init_embeddings(f2v_handle h, int kind);
/* Direct access to the embedding matrix `nCoordinates` (sample/algorithms.h:55), host N x D row-major. */
F2V_API int f2v_set_embeddings(f2v_handle h, const float *x);
F2V_API int f2v_get_embeddings(f2v_handle h, float *x_out);

/* Tunables.  "hub_chunk": neighbours per work item before a row is split (0 = never split: the
 * reference's summation order for every row; unset = chosen by f2v_train from the rows one launch covers
 * -- the batch, or a rank's slice of it in f2v_train_sharded -- or by setting "hub_chunk_for_batch" = B;
 * the chunk is part of the summation order, so pin it where bits must not depend on the number of GPUs);
 * "hub_fanin": fan-in of the tree that adds a split row's partial sums (0 = one sequential pass);
 * "merge_finalize" (default 1): the trees' nodes run in the step kernel's own grid (one launch per
 * minibatch; every in-grid wait is bounded by "tree_timeout_ms", default 5000, those of chained launches by
 * "chain_timeout_ms", default 200 -- a wait that gives up stores nothing, the launch drains, the handle falls back to 0, and
 * f2v_train repeats the call from the snapshot it took at its start; where it has none -- "recover" = 0, no room for one more
 * matrix, f2v_train_sharded, f2v_minibatch_step -- the call fails with F2V_ESTATE within an epoch or two and the embeddings
 * must be set again), 0 = one launch per tree level;
 * SINGLE TENANT: launches with in-grid waits ("merge_finalize", "chain_batches") count on this process having the GPU to
 * itself -- a second process (or a second handle of this one training at the same time) whose waiting workgroups fill the card
 * can keep the workgroups they wait for from starting; the bounded waits and "recover" turn that into a slower, correct
 * run ("recoveries" counts them), never into a hang or a wrong result.  Set both to 0 where the card is shared on purpose; f2v_create selects 0 by itself when its dispatch probe does not
 * find 8 XCDs taking workgroups round robin ("xcc_count", "xcc_round_robin" answer what it saw); "chain_batches" (default 1): f2v_train runs minibatches of up to "chain_max_batch" (4096) rows in groups of
 * "chain_rows" (65536) rows per launch, ordered by row-level data dependencies inside the launch instead of launch boundaries
 * (same results; batch 256 on RMAT-20: 0.60 -> 2.0 G edges/s); "chain_wide" (default 1): minibatches of up to "wide_max_batch" (2048) rows run
 * in the WIDE form of such launches -- the pieces of a split row meet in LDS inside one workgroup (finisher + helpers) instead of travelling
 * through HBM and combine-tree nodes, "wide_rows" (262144) rows per launch; same pieces, same fan-in groups, same results (batch 256: 2.0 -> 4.3 G
 * edges/s); needs 2 <= "hub_fanin" <= 32; "wide_phases", "wide_rounds", "wide_span", "wide_finish", "wide_order" (where a minibatch's whole-row
 * workgroups go: measured neutral), "wide_min_width" (0 = automatic) shape its
 * workgroup programs; "wide_epochs" (0 = automatic: 32 on graphs of up to 2 M nonzeros that one launch covers, else 1): that many EPOCHS of options 5 / 6 run in
 * one launch -- a ring of matrices, epoch e reads matrix e and writes matrix e + 1 behind its own row flags; same results, and what was a
 * launch boundary per epoch becomes one more hop of the dependency chain ("last_wide_epochs" answers what the last f2v_train did);
 * "wide_samples_early" (-1 = automatic: small graphs): the sample rows a launch itself writes are awaited before
 * the first neighbour waits instead of after them (placement in time only); "last_train_form" answers how the last f2v_train launched (0 one launch per minibatch, 1 chained, 2 wide, 3 hipGraph replay: set where the launches are made), "last_wide_width"
 * the sub-wave layout a wide run used, "last_wide_early" whether it ran the kernel's EARLY form; "class_cut" (default 1): a split row's pieces also end where its ascending neighbour ids cross
 * from one eighth of the id range into the next (part of the summation order, restated by the oracle; it is what makes
 * "piece_affinity" pure); "piece_affinity" (default 1): a split row's pieces run on the XCD that owns
 * the id range of their neighbours, so that each of the eight L2s caches its own eighth of the matrix (placement only:
 * results do not change; ranks of a push exchange that share one GPU switch it off by themselves); "quarter_wave": 0 selects the one-item-per-wavefront
 * kernel for every D; "waves_per_block"; "rows_in_flight" (0 = the kernels' default | 4 | 8); "use_graph" = 1 makes f2v_train replay a
 * captured hipGraph per epoch instead of launching eagerly (same results; measured no faster); "count_compulsory" = 1
 * makes new launch plans count their compulsory bytes (f2v_stats.compulsory_bytes).
 * Launch plans: the first f2v_train of a batch size builds the epoch's plans on the host (the wide form's on the host's threads:
 * F2V_IO_THREADS bounds them; RMAT-24 at batch 384: 65 plans, 0.8 s) and keeps them resident on the host and in HBM -- "plan_resident_bytes"
 * answers how much (RMAT-20 at batch 256: 184 MB; RMAT-24 at batch 384: 2.9 GB); the cache holds up to three epochs' worth of items and is
 * dropped and rebuilt on demand beyond that (a run that alternates many batch sizes).  "wide_single" = 1 (measurement only) lets the wide form run
 * launches of one minibatch.
 * Sharded runs: "push_fused" (default 1: the step kernels push their rows themselves, 0: a kernel behind
 * them does), "push_timeout_ms"; "replicate_small" (default 1): f2v_train_sharded at a batch size that f2v_train runs chained (up to
 * "chain_max_batch" rows: the reference's default 384 is one) runs the whole call on EVERY rank and exchanges nothing -- such an epoch is one
 * row-to-row dependency chain that hops over xGMI can only lengthen (sharded: 41 ms per epoch at batch 384 on two ranks; one GPU: 6.7 ms) --
 * where no two attached ranks share a GPU and every rank's GPU can chain (both learnt by f2v_push_attach, so every rank decides alike);
 * 2: also on a shared GPU; 0: never.  Bits, rand() state and the matrix every rank holds afterwards are f2v_train's.
 * f2v_get_param("last_train_replicated") tells.
 * "fast_rng" = 1 selects the NON-PARITY fast mode: initial embeddings and the option-7
 * walks are generated on the device by a counter-based RNG (same distributions, different numbers than
 * the reference's libc rand() stream); negative-sample ids still come from the handle's rand() stream.
 * f2v_get_param also answers "dim", "n", "nnz", "hub_chunk_auto" (1 while the chunk is still chosen per call), and for
 * a handle attached to a push exchange "push_rank", "push_world", "shared_card" (1: a peer runs on this very GPU). */
F2V_API int f2v_set_param(f2v_handle h, const char *name, int64_t value);
F2V_API int f2v_get_param(f2v_handle h, const char *name, int64_t *value_out);

/* ---- training --------------------------------------------------------------------------
 * Replaces vector<float> algorithms::AlgoForce2VecNS / NSBS / NSRW / NSRWBS / NSRWEFF and
 * their AVX512 twins (sample/algorithms.h:86-102; bodies sample/algorithms.cpp:544-1203,
 * 1230-4051): `iters` epochs of minibatch SGD over all N vertices in batches of `batch`,
 * drawing negative samples (and, for option 7, walks) from the handle's rand() stream in
 * the reference's order.  option: 5|6|7 (8,11 -> 5 ; 9 -> 6 with its own negative-sample range ; 10 -> 7 without the division of
 * the attraction by deg + 1, as AlgoForce2VecNSRWEFF_SREAL_D128/D64_AVXZ have it: `degi = 1.0`, sample/algorithms.cpp:2155, :3793).  bs_mode: the
 * CLI's "-bs" (1 = ns*batch samples per minibatch, row i uses samples [i, i+ns)).
 * seconds_out (may be NULL) receives the device time of the epoch loop alone (HIP events);
 * the embeddings stay in HBM (fetch with f2v_get_embeddings).  option 1 is the exact all-pairs Force2Vec (AlgoForce2Vec,
 * sample/algorithms.cpp:344-445), which samples nothing: its definition has a section of its own below. */
F2V_API int f2v_train(f2v_handle h, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode,
              double *seconds_out);
/* (While "recover" is on -- the default -- and the handle uses in-grid waits, f2v_train keeps a copy of the matrix and of the
 * rand() state as they were when the call began: one more N x D matrix of HBM, one device-to-device copy per call.  A call
 * that loses a launch is run again from there with one launch per minibatch and per tree level: same bits, F2V_OK,
 * f2v_last_error() says what happened, "recoveries" counts.) */

/* One minibatch: the kgen row-kernel boundary Calc_<pre>frc_<tdist|sigmoid>_DIM<D>_VL<V>
 * (sample/kgen/genDimFrc.base:36-57) lifted to a batch, and the unit the multi-GPU driver
 * shards.  Computes the new embeddings of rows [row_lo,row_hi) of minibatch
 * [batch_lo,batch_hi) from the pre-batch matrix into the epoch's second matrix ("staged": later
 * minibatches read them there, f2v_flush / the end of the epoch makes them the matrix; other
 * ranks' rows of the same minibatch are merged first with f2v_stage_write / an all-gather).  sample_ids: host array of the minibatch's
 * negative-sample vertex ids (ns of them, or (batch_hi-batch_lo)+ns-1 in bs_mode).
 * Option 7 uses the walks set by f2v_set_walks. */
F2V_API int f2v_minibatch_step(f2v_handle h, int option, uint32_t batch_lo, uint32_t batch_hi, uint32_t row_lo,
                       uint32_t row_hi, const uint32_t *sample_ids, uint32_t n_sample_ids, uint32_t ns, float lr,
                       int bs_mode);
/* The same step with the sample ids already in HBM: f2v_upload_sample_ids copies a host array (e.g. one
 * epoch's ids, drawn up-front: they do not depend on the embeddings) once, f2v_minibatch_step_at names the
 * minibatch's ids by their offset in it.  No host-device synchronisation per step: the multi-GPU driver
 * enqueues step and exchange back to back. */
F2V_API int f2v_upload_sample_ids(f2v_handle h, const uint32_t *ids, uint64_t count);
F2V_API int f2v_minibatch_step_at(f2v_handle h, int option, uint32_t batch_lo, uint32_t batch_hi, uint32_t row_lo,
                          uint32_t row_hi, uint64_t ids_offset, uint32_t ns, float lr, int bs_mode);
/* Commit the staged minibatch into the matrix (K5, sample/algorithms.cpp:629-639 / 913-921). */
F2V_API int f2v_flush(f2v_handle h);
/* Option 7 walk samples of the current epoch, uint32[5*n] (sample/algorithms.cpp:1097-1118). */
F2V_API int f2v_set_walks(f2v_handle h, const uint32_t *walks);
/* Draw this epoch's walks from the handle's rand() stream exactly as the reference does. */
F2V_API int f2v_generate_walks(f2v_handle h, uint32_t *walks_out /* may be NULL */);
/* randIndex(max,min) of sample/algorithms.cpp:55-58 on the handle's stream. */
F2V_API int f2v_rand_index(f2v_handle h, uint32_t max_num, uint32_t min_num, uint32_t *out);
/* `count` consecutive randIndex(max,min) draws; the first `keep` (<= count) are stored in out.
 * (One minibatch's sample loop, sample/algorithms.cpp:577-586; -bs 1 draws ns*BATCH, :686.) */
F2V_API int f2v_rand_indices(f2v_handle h, uint32_t max_num, uint32_t min_num, uint64_t count, uint64_t keep, uint32_t *out);

/* Multi-GPU exchange: device address of the staged rows of the last stepped minibatch (row r of the
 * batch at float offset (r-batch_lo)*dim; it points into the second matrix), the number of rows that may
 * be written from there (the matrix has slack behind row N for a padded all-gather), and a host
 * read/write of a row range of it (gloo / test path). */
F2V_API int f2v_stage_device_ptr(f2v_handle h, uint64_t *devptr_out, uint32_t *capacity_rows_out);
F2V_API int f2v_stage_read(f2v_handle h, uint32_t row_lo, uint32_t row_hi, float *out);
F2V_API int f2v_stage_write(f2v_handle h, uint32_t row_lo, uint32_t row_hi, const float *in);
F2V_API int f2v_stage_reserve(f2v_handle h, uint32_t rows);
/* Arbitrary rows of the matrix the staged rows live in (the epoch's second matrix), by vertex id: the
 * per-destination exchange ("send a row only to the ranks that read it") packs and unpacks with these. */
F2V_API int f2v_rows_read(f2v_handle h, const uint32_t *ids, uint32_t count, float *out);
F2V_API int f2v_rows_write(f2v_handle h, const uint32_t *ids, uint32_t count, const float *in);
/* Device address of the embedding matrix and the HIP stream (as integers) for zero-copy wrapping. */
F2V_API int f2v_embeddings_device_ptr(f2v_handle h, uint64_t *devptr_out);
F2V_API int f2v_stream(f2v_handle h, uint64_t *stream_out);
F2V_API int f2v_synchronize(f2v_handle h);

/* ---- multi-GPU: the push exchange over xGMI -----------------------------------------------
 * One process per GPU, the graph and both matrices replicated, rank r computes the r-th contiguous slice
 * of every minibatch (north_star's "1-D vertex partition ... each minibatch"; the reference has no
 * multi-device path).  What crosses GPUs is the NEW ROWS of a minibatch (forces only ever update the source
 * row): after its step kernel a rank's push kernel stores each new row straight into the second matrix of
 * every peer that READS that row -- the peers' matrices are mapped through HIP IPC, the stores travel
 * over the direct xGMI link to that peer -- and a device-side flag barrier (one small kernel, no host
 * round trip, no collective) separates minibatches.  Who reads a row is static for options 5/6: the ranks
 * owning a CSR neighbour of it, plus everyone for a vertex some minibatch samples (f2v_push_masks).
 * Results are bit-identical to the single-GPU f2v_train for any world size.
 *
 *   f2v_push_export   this rank's F2V_PUSH_EXPORT_BYTES bytes: IPC handles of both matrices and the flags, n, dim;
 *                     the host gathers them from all ranks with whatever it has (torch.distributed, MPI, a file)
 *   f2v_push_attach   map the peers (all_handles = world exports, in rank order); world <= F2V_PUSH_MAX_RANKS
 *   f2v_push_selftest every rank writes a pattern into every peer's slack rows, barrier, verifies what it
 *                     received: F2V_OK only if IPC mapping, remote stores and the flag barrier all work
 *   f2v_train_sharded f2v_train over the attached ranks (every rank calls it with the same arguments after
 *                     the same f2v_srand / f2v_init_embeddings); on return every replica is complete
 *   f2v_push_detach   unmap the peers (also done by f2v_destroy)
 * "push_timeout_ms" (f2v_set_param, default 20000) bounds every wait of the flag barrier: a missing peer
 * makes the calls fail with F2V_ESTATE instead of hanging the GPU.
 * Matrices of 2 GiB and more cannot be mapped through HIP IPC (hipIpcOpenMemHandle does not return): such
 * engines exchange through a mapped landing buffer of one minibatch (two halves of at most 512 MiB) that a
 * small kernel unpacks behind the barrier -- automatically, or for any size with "push_landing" = 1 (set
 * before f2v_push_export, on every rank alike).  A minibatch must then fit one half.
 * (Fault injection for the protocol tests lives in the self-test build only: include/f2v_test.h.) */
#define F2V_PUSH_MAX_RANKS 8
#define F2V_PUSH_EXPORT_BYTES 256
F2V_API int f2v_push_export(f2v_handle h, void *handles_out);
F2V_API int f2v_push_attach(f2v_handle h, uint32_t rank, uint32_t world, const void *all_handles);
F2V_API int f2v_push_selftest(f2v_handle h);
F2V_API int f2v_push_detach(f2v_handle h);
F2V_API int f2v_train_sharded(f2v_handle h, int option, uint32_t iters, uint32_t batch, uint32_t ns, float lr, int bs_mode,
                      double *seconds_out);
/* Host-only: the slices f2v_train_sharded cuts minibatch [lo,hi) into: bounds_out[0..world], slice r = rows
 * [bounds_out[r], bounds_out[r+1]), contiguous and balanced by work (weight of a row = its degree + 4), not by
 * row count.  (Option 7 uses equal row counts: its rows all have five pairs.) */
F2V_API int f2v_shard_bounds(const uint32_t *rowptr, uint32_t lo, uint32_t hi, uint32_t world, uint32_t *bounds_out);
/* Host-only: masks_out[v] = bit r set when rank r READS row v without owning it -- v is a CSR neighbour of a
 * row in one of r's slices (f2v_shard_bounds of every minibatch), or one of `sample_ids` (read by every row of a
 * minibatch, hence by every rank). */
F2V_API int f2v_push_masks(const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint32_t batch, uint32_t world,
                   const uint32_t *sample_ids, uint64_t n_ids, uint32_t *masks_out);
/* Rows pushed to peers / rows a full all-gather would have sent (per peer copies), since the last f2v_train_sharded began. */
F2V_API int f2v_push_stats(f2v_handle h, uint64_t *rows_pushed_out, uint64_t *rows_allgather_out);

/* Statistics of the last f2v_train: launches of the step kernel, rows and nonzeros they
 * processed, algorithmic bytes (SURVEY 8d formula), device seconds. */
typedef struct {
    uint64_t step_launches;
    uint64_t rows;
    uint64_t nnz;
    uint64_t algorithmic_bytes;
    double device_seconds;
    uint64_t hub_rows;
    uint64_t hub_chunks;
    /* with "count_compulsory" = 1: sum over the launches of (distinct embedding rows read + rows written) * 4D + 4 bytes per
     * neighbour id + 16 per work item -- the bytes a launch must move even if every re-read inside it hit a cache: the
     * numerator of a roofline fraction that cannot exceed 1 (the SURVEY 8d figure above charges every neighbour row to
     * HBM and does, on power-law graphs whose hub rows are cache hits). */
    uint64_t compulsory_bytes;
    /* (library 0.5) f2v_train keeps a snapshot of the matrix while "recover" is on and the handle's launches may hold in-grid waits:
     * one device-to-device copy of N x D floats per CALL, on the stream in front of the epoch loop and NOT part of device_seconds /
     * seconds_out -- its own device time is reported here (a caller that trains one epoch per call pays it every epoch: RMAT-20
     * ~0.2 ms, RMAT-24 ~3 ms; "recover" = 0 drops the copy and frees the matrix). */
    double snapshot_seconds;
    uint64_t recoveries;      /* give-ups f2v_train has recovered from since the handle was created ("recoveries") */
    uint32_t recovered;       /* 1: the LAST f2v_train lost a launch and ran again without in-grid waits: its device_seconds are those of
                               * the slow launch forms -- a benchmark must not quote them as the fast path's */
    uint32_t merge_finalize;  /* the handle's "merge_finalize" now: 0 after a give-up = one launch per minibatch and tree level until the
                               * in-grid waits come back (after 1, 2, 4 ... 64 healthy f2v_train calls) */
} f2v_stats;
F2V_API int f2v_get_stats(f2v_handle h, f2v_stats *out);
/* With "epoch_marks" = k > 0 the next f2v_train records a HIP event on its stream after every k-th epoch (at most 4096 of
 * them); afterwards f2v_train_marks copies the device time from the start of the epoch loop to each mark into `seconds_out`
 * (up to `cap` values; `count_out` receives how many there are): the rate over a long run second by second, without a host
 * synchronisation inside the loop. */
F2V_API int f2v_train_marks(f2v_handle h, double *seconds_out, uint32_t cap, uint32_t *count_out);

/* ---- the training objective ------------------------------------------------------------------------------------------------
 * The reference accumulates a `loglike` per epoch and never prints it (sample/algorithms.cpp:607, :621, :645); this is that
 * quantity, defined so that it is deterministic.  Evaluated at the current matrix X; lower is better; fp64 sums:
 *   positive pairs (i, j): the CSR nonzeros, duplicates included, for EVERY option -- for options 7 and 10 too the graph's edges,
 *     not an epoch's walk samples (those change every epoch and would make the curve noise);
 *   negative samples: row i has ns of them, s(i,k) = mix64(mix64(seed) ^ ((uint64)i * ns + k)) % (n - 1), k < ns -- mix64 is
 *     the splitmix64 finaliser (z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB;
 *     z ^ z>>31), seed the handle parameter "loss_seed" (default 1), the range randIndex(N-1, 0)'s, self-samples not excluded.  The
 *     handle's rand() stream is never touched (evaluating changes no later result), and the negatives are the same at every
 *     evaluation of a handle, so successive values compare;
 *   t-distribution options (5, 8, 11), the reference's own loglike expression (:607, :621):
 *     attraction = sum_(i,j) log(1 + |x_i - x_j|^2),  repulsion = -sum_(i,k) [log(1e-6 + r) - log(1 + r)],  r = |x_i - x_s(i,k)|^2;
 *   sigmoid options (6, 7, 9, 10), the function whose gradient the reference's update ascends:
 *     attraction = sum_i degi * sum_(j in N(i)) softplus(-x_i . x_j),  repulsion = sum_(i,k) softplus(x_i . x_s(i,k)),
 *     degi = 1 / (deg(i) + 1) (options 6, 7, 9: :852, :1159), 1 for option 10; softplus(z) = max(z, 0) + log1p(exp(-|z|)) exactly,
 *     not the 2048-entry sigmoid table;
 *   loss = attraction + repulsion.  A pair's squared distance / dot product is summed in fp32 (as the step kernels do), every log
 *   term and every sum in fp64.
 * The value is a function of (X, CSR, option, ns, seed) alone: bitwise identical between calls, handles and GPUs and under every
 * tunable ("waves_per_block", "quarter_wave", "rows_in_flight", "piece_affinity" ...) -- a fixed work partition (pieces of rows of
 * at most 64 neighbours, from rowptr alone) and fixed-order sums, no float atomics.  positive_pairs / negative_pairs count the
 * pairs the kernel evaluated: nnz and n * ns. */
typedef struct {
    double loss, attraction, repulsion;
    uint64_t positive_pairs, negative_pairs;
} f2v_objective_t;
/* The objective of the current matrix (pending minibatches are committed first, as f2v_get_embeddings does).  ns = 0: repulsion 0.
 * Option 1 is the exact all-pairs objective defined in its own section below (ns is ignored).
 * F2V_EINVAL for an option that is neither 1 nor one of 5..11 or a graph of fewer than two vertices, F2V_ESTATE without valid embeddings. */
F2V_API int f2v_objective(f2v_handle h, int option, uint32_t ns, f2v_objective_t *out);
/* With "loss_every" = k > 0 f2v_train also evaluates the objective -- with the call's option and ns -- after its epochs k, 2k, ...
 * and after its last epoch (at most 4096 entries per call, the first ones), on the device between the epochs: no host
 * synchronisation, the multi-epoch wide launches stay (an epoch inside one is evaluated from its matrix of the ring), and the
 * results are copied to the host once, at the end of the call.  seconds_out, f2v_stats.device_seconds and the epoch marks keep
 * their meaning, the epoch loop alone: the evaluations are bracketed by events and their time taken out; f2v_get_param
 * ("last_loss_us") answers it.  A call f2v_train runs again from its snapshot starts the log afresh.  Entry m: the 1-based epoch
 * of the call in epochs_out[m], loss / attraction / repulsion in values_out[3m .. 3m+2] (up to `cap` entries; `count_out`
 * receives how many there are).  Equal, bit for bit, to f2v_objective after training the same epochs in separate calls.
 * f2v_train_sharded with "loss_every" > 0 fails with F2V_EINVAL: a rank does not hold the whole matrix between minibatches (out
 * of scope). */
F2V_API int f2v_train_losses(f2v_handle h, uint32_t *epochs_out, double *values_out, uint32_t cap, uint32_t *count_out);

/* ---- exact all-pairs Force2Vec (option 1) -------------------------------------------------------------------------------------
 * The reference's `-option 1`, "Force2Vec (O(n^2) version)": vector<float> algorithms::AlgoForce2Vec(ITERATIONS, NUMOFTHREADS,
 * BATCHSIZE) (sample/algorithms.cpp:344-445).  Every vertex is repelled by EVERY other vertex, not by ns samples: the method the
 * options 5-11 approximate, and the ground truth they can be scored against.  f2v_train(h, 1, iters, batch, ns, lr, 0, seconds_out)
 * runs it (ns and lr are ignored: AlgoForce2Vec takes neither; bs_mode must be 0), f2v_objective(h, 1, ns, out) evaluates its
 * objective.  Defined so that the result is a function of (X, CSR, batch, epochs, first epoch) alone: bitwise identical between calls,
 * handles and GPUs and under every tunable; no float atomics.  Every operation below is one rounded fp32 operation unless it says fp64.
 *   minibatch   rows [lo, hi); every read sees the matrix as it was before the minibatch (Jacobi inside a batch, as for option 5),
 *               later minibatches see its new rows.  x is that pre-batch matrix, STEP the epoch's fp32 step;
 *   pair(i, j)  t_d = x_id - x_jd; a = the sum of t_d * t_d (rounded products) in the engine's per-pair order: the balanced
 *               adjacent-pair tree over next_pow2(D) zero-padded terms of the step kernels (ORC_ORDER_TREE of the test oracle);
 *   scale(v)    max(v, -5) then min(., 5), a NaN becoming -5: the rule of options 5 / 8 / 11;
 *   attraction  A from +0 over the CSR neighbours j of i in row order, duplicates included (:378-393):
 *               d1 = (float)(-2.0 / (1.0 + (double)a)), d2 = (float)(2.0 / ((double)a * (1.0 + (double)a))) (fp64, narrowed),
 *               f_d = scale(t_d * d1) - scale(t_d * d2), A_d = A_d + STEP * f_d;
 *   repulsion   the columns j = 0 .. n-1 are cut into pieces of F2V_EXACT_PIECE consecutive ids, the pieces into spans of
 *               F2V_EXACT_SPAN consecutive pieces.  A piece is summed from +0 in ascending j, skipping j == i:
 *               P_d = P_d + STEP * scale(t_d * d1), d1 = (float)(2.0 / ((double)a * (1.0 + (double)a))) (:395-422); a span is the
 *               sequential sum from +0 of its piece sums in ascending order; nothing is added for a column past n - 1;
 *   row         Y = A, then Y = Y + S_s for the spans s in ascending order; the new x_i = x_i + Y (:429-431);
 *   epochs      STEP_0 = 1.0f, STEP_(e+1) = (float)((double)STEP_e * 0.999) (:436).  The handle parameter "exact_epoch" (default 0,
 *               get and set) is the index e of the next call's first epoch, STEP_e formed by e such multiplications; a call of
 *               `iters` epochs advances it by `iters`: two calls of 5 epochs equal one of 10 bit for bit, setting it to 0 starts over;
 *   rand()      no draw is made: the handle's stream stays where it was.
 * (The reference sums a row in one fp32 accumulator: neighbours, then j < i, then j > i.  The pieces and spans are what lets the
 * n columns of a row be summed side by side; after a few epochs the two orders differ by some 1e-5: DESIGN.md section 14.)
 * Launches: per minibatch one pair kernel (grid: groups of "exact_rows" rows -- 0 = automatic | 4 | 8 | 16, placement only, it never
 * changes a bit -- times spans + 1 slices; where D is a multiple of 4 up to 256 and "quarter_wave" is on, minibatches of
 * "exact_quarter_min" rows or more, default 1024, 0 = all, run it in the quarter-wave layout: the same bits; "last_exact_rows" and
 * "last_exact_quarter" answer what the last minibatch ran with) and one finish kernel, plain launches on the handle's stream without in-grid waits: no
 * snapshot is taken, nothing is recovered, "last_train_form" answers 0.  seconds_out, f2v_stats.device_seconds and "epoch_marks" keep
 * their meaning; step_launches counts the pair kernel's launches, rows the rows updated, nnz the CSR nonzeros visited.  Workspace,
 * allocated on first use (grown for a larger minibatch) and freed by f2v_destroy: min(batch, n) x (spans + 1) x D floats, spans =
 * ceil(n / (F2V_EXACT_PIECE * F2V_EXACT_SPAN)) -- a row's span sums and its attraction part.
 * Single GPU, f2v_train only: f2v_train_sharded, f2v_minibatch_step and f2v_minibatch_step_at answer option 1 with F2V_EINVAL.
 * The objective, f2v_objective(h, 1, ns ignored, out), the reference's own loglike of this function (:387, :407, :416; EPS 1e-6):
 *   attraction = sum over the nonzeros (i, j) of flog(1 + a),  repulsion = -sum over all ordered pairs i != j of
 *   [flog(1e-6 + a) - flog(1 + a)],  positive_pairs = nnz, negative_pairs = n (n - 1), loss = attraction + repulsion;
 *   a is the fp32 pair sum above, converted exactly; everything else is fp64.  flog(v), for the positive normal numbers that occur
 *   here, is the natural logarithm computed from rounded fp64 additions, multiplications and one division in this order (fdlibm's
 *   e_log.c without its special cases; within 1 ulp of log): v = 2^k * m with m in [1, 2); if m > 1.4142135623730951 then m = m * 0.5
 *   and k = k + 1; f = m - 1; s = f / (2 + f); z = s * s; w = z * z; t1 = w * (L2 + w * (L4 + w * L6)); t2 = z * (L1 + w * (L3 + w *
 *   (L5 + w * L7))); R = t2 + t1; h = (0.5 * f) * f; flog = k * 6.93147180369123816490e-01 - ((h - (s * (h + R) + k *
 *   1.90821492927058770002e-10)) - f); L1 .. L7 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01,
 *   2.222219843214978396e-01, 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01 -- so that a host
 *   restatement reproduces the value bit for bit (a library's log differs from another's in the last place);
 *   order of the fp64 sums: per row, the repulsion terms in pieces of 64 columns, each from +0 in ascending j skipping i, the piece
 *   sums added sequentially from +0 in ascending order; the attraction terms of a row likewise in pieces of 64 neighbours in row
 *   order; the row sums in pieces of 64 consecutive rows, each from +0, and those piece sums sequentially from +0.
 * "loss_every" / f2v_train_losses work for option 1 with the same guarantee as for the others: equal, bit for bit, to f2v_objective
 * after the same epochs in separate calls.  Workspace of the objective: 2 n + 2 ceil(n / 64) doubles.
 * The two constants are part of the summation order. */
#define F2V_EXACT_PIECE 64 /* columns per piece */
#define F2V_EXACT_SPAN 16  /* pieces per span: 1024 columns */

/* ---- nearest neighbours ---------------------------------------------------------------------------------------------------
 * Which rows of the matrix are most similar to a query?  Three similarities between a query vector q and row c of the matrix, all
 * fp32, all "larger is nearer".  fma(a, b, acc) is one correctly rounded fp32 fused multiply-add; a chain starts from +0 and runs
 * over d = 0 .. D-1 in ascending order:
 *   F2V_SIM_DOT     s = chain_d fma(q_d, c_d, acc);
 *   F2V_SIM_L2      s = -chain_d fma(t_d, t_d, acc), t_d = q_d - c_d (one rounded subtraction) -- always from differences, never
 *                   |q|^2 + |c|^2 - 2 q.c: that form cancels for exactly the pairs a nearest-neighbour query is about;
 *   F2V_SIM_COSINE  s = (dot * r_q) * r_c (two rounded multiplications), dot as above, r_v = 1 / sqrt(n_v), n_v = chain_d fma(v_d, v_d,
 *                   acc), square root and division correctly rounded, r_v = 0 where n_v == 0.  Where n_v overflows, r_v = 1 / sqrt(inf)
 *                   = 0 by that very arithmetic: the score is a zero where dot is finite and a NaN where dot is infinite (inf x 0).
 * Subnormals are kept.  Ranking is a strict total order: score descending (-0 and +0 are one score), equal scores by ascending
 * vertex id, a NaN score below every number (NaNs among themselves by ascending id).  A query's result is the first k candidates of
 * that order after the exclusions; where fewer than k are left the tail holds id 0xFFFFFFFF and score -inf.  The result is a function
 * of the matrix, the metric, k and the flags alone: never of how many queries share a call, of "nearest_splits" / "nearest_block" /
 * "nearest_chunk" (f2v_set_param), of the handle or of the order in which workgroups run.  dot and cosine are computed by the fp32
 * matrix instruction v_mfma_f32_32x32x2_f32, whose accumulator is that very chain; L2 by the vector ALU.
 * All three work on the matrix as f2v_get_embeddings would return it (pending minibatches are committed first), run on the
 * handle's stream behind whatever training was enqueued, and change neither the matrices nor the rand() stream nor any later
 * training result.  Any nq: queries run in chunks of "nearest_chunk" (default 8192); the N x nq scores are never stored, the
 * workspace is chunk x splits x k keys, allocated on first use and freed by f2v_destroy.  seconds_out (may be NULL): device time
 * between events around the query's own launches, uploads and downloads excluded.  On a handle attached to a push exchange it reads
 * this rank's replica; nothing is exchanged.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers, k = 0 or k > F2V_NEAREST_MAX_K, an unknown metric or flag, a query
 * id >= n, and -- for F2V_NEAREST_EXCLUDE_NEIGHBOURS and f2v_neighbour_recall, which search CSR rows -- a CSR whose column ids
 * are not ascending inside every row (the order f2v_create documents; checked once per handle).  nq = 0 is F2V_OK and touches
 * nothing: no launch, no commit of pending minibatches. */
#define F2V_SIM_DOT 0
#define F2V_SIM_L2 1
#define F2V_SIM_COSINE 2
#define F2V_NEAREST_MAX_K 128
#define F2V_NEAREST_EXCLUDE_SELF 1u       /* drop the query vertex itself */
#define F2V_NEAREST_EXCLUDE_NEIGHBOURS 2u /* drop the query vertex's CSR neighbours ("similar, but not linked yet") */
/* Queries are rows of the matrix.  ids_out: nq x k; scores_out: nq x k, may be NULL. */
F2V_API int f2v_nearest_rows(f2v_handle h, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint32_t flags, uint32_t *ids_out,
                     float *scores_out, double *seconds_out);
/* Queries are caller-supplied vectors, nq x D fp32 on the host (there is no query vertex, hence no flags). */
F2V_API int f2v_nearest_vectors(f2v_handle h, const float *queries, uint32_t nq, uint32_t k, int metric, uint32_t *ids_out, float *scores_out,
                        double *seconds_out);
/* Graph-reconstruction precision@k over the given vertices (query_ids NULL: all n, nq ignored), counted on the device:
 * hits = sum_v |top-k(v) n N(v)| with v itself excluded from its top-k, possible = sum_v min(k, d(v)), d(v) the number of DISTINCT
 * neighbours of v other than v (duplicate nonzeros and self-loops of the CSR count once / not at all). */
F2V_API int f2v_neighbour_recall(f2v_handle h, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint64_t *hits_out,
                         uint64_t *possible_out, double *seconds_out);

/* ---- clustering ------------------------------------------------------------------------------------------------------------
 * The third score the reference judges an embedding by (performancescores/runnodeclassclust.py:311-331): k-means on the rows of the
 * matrix, then the modularity of that clustering on the input graph -- the one score that needs no labels.  Lloyd's iteration,
 * defined so that it is deterministic; fma(a, b, acc) is one correctly rounded fp32 fused multiply-add:
 *   distance    dist(x, c) = chain_d fma(t_d, t_d, acc) from +0 over ascending d, t_d = x_d - c_d (one rounded subtraction): -F2V_SIM_L2
 *               of the nearest-neighbour definition above, always from differences, subnormals kept;
 *   assignment  label(v) = the centroid of smallest dist, ties to the lowest centroid index, a NaN distance after every number
 *               (all NaN: label 0): the ranking of f2v_nearest_* over the K centroids with k = 1;
 *   update      the members of cluster c in ascending vertex id, cut into pieces of F2V_KMEANS_PIECE consecutive members; a piece is
 *               summed per dimension in fp64, sequentially from +0; the piece sums are added sequentially in ascending piece order
 *               in fp64; centroid_d = (float)(sum_d / (double)count); a cluster without members keeps its previous centroid;
 *   inertia     the fp64 sum of the fp32 distances dist(v, centroid[label(v)]): vertices in ascending id in pieces of 64 consecutive
 *               vertices summed sequentially from +0, the piece sums added sequentially in ascending order;
 *   iteration   with C_0 the initial centroids, for t = 1, 2, ...: L_t = assign(X, C_(t-1)); if t > 1 and L_t == L_(t-1) stop with
 *               converged = 1, iterations = t - 1; if t - 1 == max_iters stop with converged = 0, iterations = max_iters;
 *               C_t = update(X, L_t, C_(t-1)).  Returned are L_t, C_(t-1), the inertia of that pair and the member counts of L_t,
 *               so labels == assign(X, centroids) always holds; max_iters = 0 is a pure assignment to the given centroids;
 *   initial centroids   k x D floats from the caller, or seeded rows: key(v) = mix64(mix64(seed) ^ v) (mix64: the splitmix64
 *               finaliser of the objective above), vertices sorted by key ascending, ties by id, centroid c = the row of the c-th
 *               vertex of that order (k distinct vertices).  Restart r of `restarts` (0-based) uses seed + r; the result is the
 *               restart of lowest inertia (fp64 compare), ties to the lowest r.
 * The result is a function of (X, k, max_iters, restarts, seed or the given centroids) alone: never of launch shapes, of
 * "kmeans_block" (f2v_set_param: rows per workgroup of the assignment kernel, 0 = automatic | 64 | 128 | 256) or any other tunable,
 * of the handle or of the order in which workgroups run; no float atomics.
 * f2v_kmeans works on the matrix as f2v_get_embeddings would return it (pending minibatches are committed first), runs on the
 * handle's stream and changes neither the matrices nor the rand() stream nor any later training result; on a handle attached to a
 * push exchange it reads this rank's replica.  Workspace, allocated on first use (grown for a larger k) and freed by f2v_destroy:
 * 4 n-word arrays (labels, the best restart's labels, the members in cluster order, distances), 2 k x D floats, ceil(n / 1024) x k
 * words of block histograms, (n / 64 + k) x D doubles of piece sums and ceil(n / 64) doubles of inertia pieces.  The convergence
 * test reads 4 bytes back per iteration.  info_out->seconds: device time between events around the call's own launches.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers, k = 0, k > F2V_KMEANS_MAX_K, k > n, restarts = 0, and
 * restarts > 1 together with init_centroids. */
#define F2V_KMEANS_MAX_K 1024
#define F2V_KMEANS_PIECE 64
typedef struct {
    double inertia;
    double seconds;
    uint32_t iterations, converged, restart, reserved;
} f2v_kmeans_t;
F2V_API int f2v_kmeans(f2v_handle h, uint32_t k, uint32_t max_iters, uint32_t restarts, uint64_t seed,
               const float *init_centroids /* k x D or NULL */, uint32_t *labels_out /* n */, float *centroids_out /* k x D, may be NULL */,
               uint64_t *counts_out /* k, may be NULL */, f2v_kmeans_t *info_out);
/* Newman modularity of a labelling (labels[v] < n_clusters) on the SIMPLE undirected graph of the CSR: every unordered pair {u, v}
 * that occurs as a nonzero in either direction counts once (duplicates are collapsed), a self-loop is one edge and adds 2 to its
 * vertex's degree; m = edges, inside[c] = edges with both ends in c, degree[c] = sum of the simple-graph degrees of c's vertices;
 * Q = sum over c ascending of (inside[c] / m - (degree[c] / (2 m))^2) in fp64, sequentially, 0 when m = 0.  The tallies are integers
 * counted on the device with integer atomics (exact, independent of order), Q is formed on the host from them.  Needs no embeddings.
 * The last three outputs may be NULL (inside_out, degree_out: n_clusters values each).  F2V_EINVAL for null pointers, n_clusters = 0,
 * a label >= n_clusters and a CSR whose column ids are not ascending inside every row (rows are searched; checked once per handle). */
F2V_API int f2v_modularity(f2v_handle h, const uint32_t *labels /* n */, uint32_t n_clusters, double *q_out, uint64_t *edges_out,
                   uint64_t *inside_out, uint64_t *degree_out);

/* ---- nearest neighbours through an index ---------------------------------------------------------------------------------------
 * f2v_nearest_* score every query against all n rows.  An inverted-file index looks only where the answer can be: the rows are
 * partitioned once, and a query scores the rows of the few lists whose centroids are nearest.  It is EXACT top-k over a well-defined
 * candidate set, so the rule that a result is a function of its inputs alone, bit for bit, holds here too.
 *   index       a partition of the n vertices into `lists` lists, labels[v] < lists, plus one centroid of D floats per list;
 *               1 <= lists <= min(n, F2V_INDEX_MAX_LISTS).  The members of list c are the vertices with labels[v] == c in ascending
 *               id; an empty list is legal.
 *   build       k-means form: labels and centroids are exactly what f2v_kmeans(h, lists, max_iters, 1, seed, init_centroids, ...)
 *               returns on the matrix as it stands, bit for bit -- it IS that call, not a second k-means; info reports its inertia,
 *               iterations and converged.  Given form: the caller supplies labels (n words) and centroids (lists x D floats, any
 *               values); nothing requires a vertex to lie in the list of its nearest centroid, the definition below does not care.
 *   ownership   the index lives in buffers of its own inside the handle (labels, members in list order, lists + 1 offsets,
 *               centroids: info.bytes), not in the growable workspaces that f2v_kmeans, f2v_silhouette and the other scorers
 *               overwrite: later f2v_kmeans calls, training and f2v_set_embeddings leave it alone.  A second build replaces it;
 *               f2v_index_drop and f2v_destroy free it.
 *   no copy     THE INDEX HOLDS NO COPY OF THE MATRIX.  Scores, and the vectors of queries given by id, always come from the matrix as
 *               f2v_get_embeddings would return it at the time of the search (pending minibatches are committed first).  Training or
 *               f2v_set_embeddings after a build makes the PARTITION stale: that costs recall and never makes a result ill-defined.
 *               Nothing rebuilds the index by itself and nothing tracks its age.
 *   search      scores, metrics, flags, ranking order and padding (id 0xFFFFFFFF, score -inf) are those of "nearest neighbours"
 *               above, unchanged.  For a query q and nprobe, P = min(nprobe, lists).  The probed lists are the first P entries of the
 *               result order f2v_nearest_vectors gives for q over the lists x D centroid matrix with the call's metric and k = P
 *               (score descending, ties to the lower list index, a NaN score last, cosine with r = 0 for a zero centroid; an empty
 *               list is ranked like any other).  The candidates are the members of the probed lists; the result is the first k
 *               candidates, after the exclusions, in the nearest-neighbour order.  1 <= nprobe <= F2V_INDEX_MAX_PROBES,
 *               1 <= k <= F2V_NEAREST_MAX_K.  probes_out (nq x P, may be NULL) receives the probed lists in probe order.
 * Consequences:
 *   (a) the result is a function of (X, labels, centroids, metric, k, nprobe, flags, query) alone: never of how many queries share a
 *       call, of how (query, list) pairs are grouped into workgroups, of "index_chunk" (queries per launch, default 8192),
 *       "index_split_tiles" (tiles of 128 candidates per work item of the scan, default 8), "index_block" (queries per work item of
 *       the scan: 0 = 128 where D <= 128 and a list has more than 32 queries left, else 32 | 32) or any other tunable, of the handle, or
 *       of the order in which workgroups or atomics land (the only atomics are integer counters that place work);
 *   (b) with nprobe >= lists (possible for lists <= 128) ids and scores equal f2v_nearest_rows / f2v_nearest_vectors bit for bit;
 *   (c) per query the probed lists at nprobe = p are a prefix of those at p + 1, so the number of true top-k ids found never falls
 *       as nprobe rises.
 * f2v_index_search_t: seconds -- device time between events around the call's own launches; nprobe -- the P used; candidates -- the
 * sum over the queries of the member counts of their probed lists (an integer function of the inputs).  f2v_index_t: the k-means
 * form's inertia / iterations / converged (0 in the given form), seconds (the k-means and the counting sort into list order), bytes
 * (device bytes the index holds), lists, largest (members of the longest list), empty (lists without members).
 * No call touches the matrices, the rand() stream or any later training result; all run on the handle's stream; on a handle attached
 * to a push exchange they read this rank's replica.  The searches' workspace (one query chunk: vectors, probes, buckets, work items,
 * chunk x P x ranges x k keys, capped at 2^24 keys by running fewer queries per launch) is allocated on first use and freed by
 * f2v_destroy.
 * F2V_ESTATE: a search or f2v_index_get without an index, a k-means build without valid embeddings.  F2V_EINVAL: the
 * nearest calls' conditions, lists = 0, lists > n or lists > F2V_INDEX_MAX_LISTS, a label >= lists, nprobe = 0 or nprobe >
 * F2V_INDEX_MAX_PROBES, null labels or centroids in the given form.  nq = 0 is F2V_OK and touches nothing. */
#define F2V_INDEX_MAX_LISTS 1024 /* == F2V_KMEANS_MAX_K */
#define F2V_INDEX_MAX_PROBES 128 /* == F2V_NEAREST_MAX_K */
typedef struct {
    double inertia, seconds;
    uint64_t bytes;
    uint32_t lists, iterations, converged, largest, empty, reserved;
} f2v_index_t;
typedef struct {
    double seconds;
    uint64_t candidates;
    uint32_t nprobe, reserved;
} f2v_index_search_t;
F2V_API int f2v_index_build(f2v_handle h, uint32_t lists, uint32_t max_iters, uint64_t seed, const float *init_centroids /* lists x D or NULL */,
                    f2v_index_t *info_out /* may be NULL */);
F2V_API int f2v_index_build_given(f2v_handle h, const uint32_t *labels /* n */, const float *centroids /* lists x D */, uint32_t lists,
                          f2v_index_t *info_out /* may be NULL */);
/* The index as it stands: labels (n), centroids (lists x D), member counts (lists) and the build's info; each output may be NULL. */
F2V_API int f2v_index_get(f2v_handle h, uint32_t *labels_out, float *centroids_out, uint64_t *counts_out, f2v_index_t *info_out);
/* Frees the index; F2V_OK where there is none. */
F2V_API int f2v_index_drop(f2v_handle h);
/* Queries are rows of the matrix.  ids_out: nq x k; scores_out: nq x k, may be NULL; probes_out: nq x P, may be NULL; info_out may be NULL. */
F2V_API int f2v_index_search_rows(f2v_handle h, const uint32_t *query_ids, uint32_t nq, uint32_t k, int metric, uint32_t flags, uint32_t nprobe,
                          uint32_t *ids_out, float *scores_out, uint32_t *probes_out, f2v_index_search_t *info_out);
/* Queries are caller-supplied vectors, nq x D fp32 on the host (no query vertex, hence no flags). */
F2V_API int f2v_index_search_vectors(f2v_handle h, const float *queries, uint32_t nq, uint32_t k, int metric, uint32_t nprobe, uint32_t *ids_out,
                             float *scores_out, uint32_t *probes_out, f2v_index_search_t *info_out);

/* ---- logistic regression -----------------------------------------------------------------------------------------------------
 * The other two scores the reference judges an embedding by: node-classification F1 (performancescores/runnodeclassclust.py:289-309)
 * and link-prediction accuracy / F1 (performancescores/runlinkpredict.py:127-140) are both an L2-regularised one-vs-rest logistic
 * regression, fitted on rows of the matrix or on per-pair features of two rows.  fma(a, b, acc) is one correctly rounded fp64 fused
 * multiply-add.
 *   samples     m of them; sample i is the vertex a[i] with feature vector f_i = row a[i] (b_ids == NULL), or the pair (a[i], b[i])
 *               with f_i formed per dimension in fp32, one rounding per operation (runlinkpredict.py:63-72): F2V_PAIR_HADAMARD
 *               x_a * x_b, F2V_PAIR_L1 |x_a - x_b|, F2V_PAIR_L2 t * t with t = x_a - x_b, F2V_PAIR_AVERAGE (x_a + x_b) * 0.5f;
 *               subnormals kept; duplicate ids and a == b are legal;
 *   targets     y: m x C bytes of 0 / 1, one column per class (several columns of a sample may be 1), 1 <= C <= F2V_LOGREG_MAX_CLASSES;
 *   objective   every class c is a problem of its own over (w_c in R^D, b_c), in fp64, the features converted exactly:
 *               z_ic = the chain fma(f_id, w_cd, acc) from +0 over ascending d, then + b_c;
 *               softplus(z) = max(z, 0) + log1p(exp(-|z|)) (as in the objective above), sigma(z) = 1 / (1 + exp(-z)) for z >= 0,
 *               exp(z) / (1 + exp(z)) below; r_ic = sigma(z_ic) - y_ic; l_ic = softplus(z_ic) - y_ic * z_ic;
 *               J_c = 0.5 * lambda * sum_d w_cd^2 + sum_i l_ic;  dJ/dw_cd = lambda * w_cd + sum_i r_ic * f_id;  dJ/db_c = sum_i r_ic
 *               (the bias is not regularised: scikit-learn's lbfgs);
 *   sums        every sum over samples has one order: the samples in the caller's order are cut into blocks of F2V_LOGREG_BLOCK
 *               consecutive samples; a block is summed sequentially from +0 -- sum_i r_ic * f_id as fma(r_ic, f_id, acc), the
 *               others by addition; the block sums are added sequentially from +0 in ascending block order.  The regulariser is
 *               formed on the host: q_c = the chain fma(w_cd, w_cd, acc) from +0 over ascending d, J_c = fma(0.5 * lambda, q_c,
 *               sum_i l_ic), dJ/dw_cd = fma(lambda, w_cd, sum_i r_ic * f_id).  No float atomics.
 * Results are a function of (X, samples, y, weights, lambda) alone: never of launch shapes, of a tunable, of the handle or of the order
 * in which workgroups run, and bitwise identical between calls, handles and GPUs.
 *   solver      f2v_logreg_fit minimises every J_c on the host in plain fp64, deterministically, each class with an L-BFGS state of
 *               its own: start W = 0, b = 0; the last 10 pairs (s, y) of accepted steps, a pair with s.y <= 0 dropped; the direction
 *               from the two-loop recursion scaled by s.y / y.y of the newest pair (steepest descent without pairs, or where the
 *               recursion's direction does not descend: the pairs are dropped then); trial step 1 / ||g||_1 in a class's first
 *               iteration, 1 afterwards; Armijo backtracking J(x + t p) <= J(x) + 1e-4 t g.p, halving t at most 40 times -- a
 *               class whose line search fails stops where it is with converged = 0; a class stops with converged = 1 once
 *               ||g||_inf <= tol * m (scikit-learn's test on its objective J / m), and at max_iter iterations (accepted steps).
 *               All classes still active take their trial points in the same device pass: one pass over the samples serves every
 *               class.  lambda = 1, tol = 1e-4, max_iter = 100 are LogisticRegression()'s C = 1 and defaults.
 * The three calls work on the matrix as f2v_get_embeddings would return it (pending minibatches are committed first), run on the
 * handle's stream and change neither the matrices nor the rand() stream nor any later training result; on a handle attached to a
 * push exchange they read this rank's replica.  Weights are classes x (D + 1) doubles, a class's bias last.  Workspace, allocated on
 * first use (grown for a larger call) and freed by f2v_destroy: the ids (2 m words), the targets (m x C bytes), ceil(m / 1024) x C x
 * (D + 2) doubles of block sums (a class's D + 1 gradient sums and its loss), 2 x C x (D + 2) doubles of weights and results, and for
 * f2v_logreg_decision min(m, 262144) x C doubles.  seconds: device time between events around the call's own launches.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers, m = 0, classes = 0 or > F2V_LOGREG_MAX_CLASSES, an id >= n, a
 * target byte above 1, an unknown feature (pairs), a negative or NaN lambda, tol <= 0 or NaN. */
#define F2V_LOGREG_MAX_CLASSES 64
#define F2V_LOGREG_BLOCK 1024
#define F2V_PAIR_HADAMARD 0
#define F2V_PAIR_L1 1
#define F2V_PAIR_L2 2
#define F2V_PAIR_AVERAGE 3
typedef struct {
    double loss;       /* J_c at the returned weights */
    double gnorm_inf;  /* ||grad J_c||_inf there */
    double seconds;    /* device time of the whole call's launches (the same in every class's entry) */
    uint32_t iterations, evaluations, converged, reserved;
} f2v_logreg_t;
/* One pass: loss_out[c] = J_c and grad_out[c] = (dJ/dw_c, dJ/db_c) of every class at the given weights. */
F2V_API int f2v_logreg_eval(f2v_handle h, const uint32_t *a_ids, const uint32_t *b_ids /* NULL: row samples */, uint32_t m, int feature,
                    const uint8_t *y /* m x classes */, uint32_t classes, const double *weights /* classes x (D + 1) */, double lambda,
                    double *loss_out /* classes */, double *grad_out /* classes x (D + 1) */, double *seconds_out /* may be NULL */);
F2V_API int f2v_logreg_fit(f2v_handle h, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const uint8_t *y,
                   uint32_t classes, double lambda, double tol, uint32_t max_iter, double *weights_out /* classes x (D + 1) */,
                   f2v_logreg_t *info_out /* classes */);
/* z_out[i][c] = z_ic of the definition for the given samples and weights; argmax, top-k and F1 are the host's business. */
F2V_API int f2v_logreg_decision(f2v_handle h, const uint32_t *a_ids, const uint32_t *b_ids, uint32_t m, int feature, const double *weights,
                        uint32_t classes, double *z_out /* m x classes */, double *seconds_out /* may be NULL */);

/* ---- separation ------------------------------------------------------------------------------------------------------------------
 * The fourth score the reference judges an embedding by (performancescores/runvisualization.py prints "silhouette: <x>
 * davies_bouldin: <y>"): how well a labelling -- ground truth, or the clusters of f2v_kmeans -- separates in the embedding space.
 * They are scikit-learn's silhouette_score(X, labels) and davies_bouldin_score(X, labels) with the Euclidean metric, defined so that
 * they are deterministic; fma and dist are those of the clustering definition above:
 *   labelling   labels[v] < n_clusters, or F2V_LABEL_NONE: such a vertex takes no part, neither as a sample nor as a member of any
 *               cluster (the reference's script gives unlabelled vertices a cluster of their own, -1; this definition leaves them out);
 *   distance    d(x, c) = sqrtf(dist(x, c)): dist is the fp32 chain fma(t_d, t_d, acc) from +0 over ascending d with t_d = x_d - c_d
 *               (one rounded subtraction), the square root one correctly rounded fp32 operation; subnormals kept; always from
 *               differences, never as |x|^2 + |c|^2 - 2 x.c;
 *   members     the members of cluster c are the vertices with labels[v] == c in ascending vertex id, n_c of them; they are cut into
 *               pieces of F2V_SEPARATION_PIECE consecutive members, the pieces into spans of F2V_SEPARATION_SPAN consecutive pieces;
 *   cluster sum sum_c(i) = the fp64 sum of the fp32 distances d(x_i, x_j) over the members j of c (i itself included where it is a
 *               member: its distance is +0): a piece is summed sequentially from +0 in member order, the piece sums of a span are
 *               added sequentially from +0 in ascending order, a cluster's span sums are added sequentially from +0 in ascending
 *               order.  Nothing is added for a place past a cluster's last member;
 *   silhouette  with L = labels[i]: a(i) = sum_L(i) / (double)(n_L - 1); b(i) = the smallest m = sum_c(i) / (double)n_c over the
 *               non-empty clusters c != L, taken in ascending c and replaced only where m < b, other(i) = that c;
 *               s(i) = (b - a) / max(a, b) with max(a, b) = a > b ? a : b; s(i) = 0 where n_L == 1 or max(a, b) == 0;
 *   score       the samples in the caller's order (sample_ids == NULL: every labelled vertex in ascending id) are cut into pieces of
 *               64; the s(i) of a piece are added sequentially from +0, the piece sums are added sequentially from +0 in ascending
 *               order, the result is divided by the number of samples.  A sample is scored against ALL labelled vertices (scikit-
 *               learn's sample_size scores a sample against the other samples only); duplicate sample ids are legal;
 *   Davies-Bouldin   centroid_c of a non-empty cluster = the k-means update above ((float)(fp64 sum in pieces of 64 members / n_c));
 *               S_c = the fp64 sum of d(x_v, centroid_c) over the members in the piece / span order above, divided by (double)n_c;
 *               M_cd = (double)d(centroid_c, centroid_d) on the fp32 centroids; R_cd = 0 where S_c + S_d == 0, else (S_c + S_d) /
 *               M_cd (+inf for coincident centroids); the score is the sequential fp64 sum over the non-empty clusters c ascending
 *               of max over the non-empty d != c of R_cd (taken in ascending d, replaced only where R > max), divided by their
 *               number.  Departures from scikit-learn: fp32 distances and centroids instead of fp64 ones; its early `return 0.0`
 *               where all centroid distances are close to zero is not reproduced (coincident centroids give +inf here, 0 only
 *               where the scatters vanish too); an empty cluster id below n_clusters is simply not a cluster (scikit-learn
 *               re-encodes the labels); centroids_out and scatter_out hold zeros for an empty cluster.
 * Results are a function of (X, labels, samples) alone: never of launch shapes, of "separation_chunk" (f2v_set_param: samples per
 * launch, default 8192), of "separation_block" (sample rows per workgroup, 0 = automatic | 64 | 128) or of any other tunable, of the
 * handle or of the order in which workgroups run; no float atomics; bitwise identical between calls, handles and GPUs.
 * Both calls work on the matrix as f2v_get_embeddings would return it (pending minibatches are committed first), run on the
 * handle's stream and change neither the matrices nor the rand() stream nor any later training result; on a handle attached to a
 * push exchange they read this rank's replica.  Workspace, allocated on first use (grown for a larger call) and freed by f2v_destroy:
 * the clustering workspace of f2v_kmeans for n_clusters (its counting sort, centroids and piece sums are used), the labelled
 * vertices (n words), per sample 3 words and a double, ceil(samples / 64) doubles of score pieces, per span 2 words, and
 * min(samples, "separation_chunk") x spans doubles of span sums, spans = sum over c of ceil(n_c / 4096) <= n / 4096 + n_clusters:
 * one double per (sample, span).  seconds: device time between events around the call's own launches.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers (labels, score_out), n_clusters = 0 or above
 * F2V_SEPARATION_MAX_CLUSTERS, a label that is neither below n_clusters nor F2V_LABEL_NONE, a sample id >= n or one whose label is
 * F2V_LABEL_NONE, nq = 0 together with sample_ids, fewer than two non-empty clusters, and for the silhouette as many non-empty
 * clusters as labelled vertices (scikit-learn's 2 <= n_labels <= n_samples - 1). */
#define F2V_LABEL_NONE 0xFFFFFFFFu         /* the vertex takes no part: neither a sample nor a member of any cluster */
#define F2V_SEPARATION_MAX_CLUSTERS 1024
#define F2V_SEPARATION_PIECE 64            /* members per piece */
#define F2V_SEPARATION_SPAN 64             /* pieces per span: 4096 members */
F2V_API int f2v_silhouette(f2v_handle h, const uint32_t *labels /* n */, uint32_t n_clusters,
                   const uint32_t *sample_ids /* NULL: every labelled vertex, ascending id */, uint32_t nq,
                   double *s_out /* per sample, may be NULL */, uint32_t *other_out /* per sample: the cluster of b(i), may be NULL */,
                   double *score_out, double *seconds_out /* may be NULL */);
F2V_API int f2v_davies_bouldin(f2v_handle h, const uint32_t *labels, uint32_t n_clusters, double *score_out,
                       float *centroids_out /* n_clusters x D, may be NULL */, double *scatter_out /* n_clusters, may be NULL */,
                       uint64_t *counts_out /* n_clusters, may be NULL */, double *seconds_out /* may be NULL */);

/* ---- layout ----------------------------------------------------------------------------------------------------------------------
 * The step that gives performancescores/runvisualization.py its name (:177-181, :190-198): reduce the embedding to two dimensions, say
 * how faithful the picture is ("TrustWorthiness: <x>"), write the coordinates out.  The script's t-SNE is O(n^2) per iteration and
 * chaotic; the deterministic answer is a principal-component projection, and the score is scikit-learn's trustworthiness itself, between
 * the matrix and ANY second matrix over the same vertices.
 *
 * f2v_pca -- all fp64; fma(a, b, acc) is one correctly rounded fp64 fused multiply-add:
 *   mean        the vertices in ascending id are cut into pieces of F2V_PCA_PIECE consecutive vertices; a piece is summed per dimension
 *               sequentially from +0 (the floats converted exactly), the piece sums are added sequentially from +0 in ascending piece
 *               order, mean_d = sum_d / (double)n;
 *   scatter     S_de for d <= e from z_vd = (double)x_vd - mean_d (one rounded subtraction): within a piece the chain fma(z_vd, z_ve,
 *               acc) from +0 in ascending vertex id, the piece sums added sequentially from +0 in ascending piece order; S_ed = S_de;
 *   eigenvectors   the cyclic Jacobi method on S, every product and sum one rounded fp64 operation, no fma: A = S, V = I; a sweep visits
 *               (p, q) for p = 0 .. D-2, q = p+1 .. D-1; a_pq == 0: the pair is skipped; |a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq|
 *               == |a_qq|: a_pq = a_qp = 0 and the pair is skipped; else theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| +
 *               sqrt(theta * theta + 1)) with sgn(theta) = +1 where theta >= 0 and -1 otherwise, c = 1 / sqrt(t * t + 1), s = t * c; rows
 *               p and q of A become c a_p. - s a_q. and s a_p. + c a_q. (from the old rows), then columns p and q are updated the same
 *               way, a_pq = a_qp = 0, and columns p and q of V are updated the same way: a rotation.  The method stops after the first
 *               sweep without a rotation (converged = 1) and in any case after 64 sweeps (converged = 0); sweeps counts the sweeps run,
 *               the one without a rotation included;
 *   order, sign eigenpairs by eigenvalue (the diagonal of A) descending, ties by ascending original column, a NaN after every number; a
 *               component is negated where its entry of largest magnitude is negative (the lowest d among equal magnitudes);
 *   projection  y_vc = (float) of the chain fma(z_vd, w_cd, acc) from +0 over ascending d, c < d2, z_vd the difference above;
 *   outputs     y_out n x d2 floats, components_out d2 x D, mean_out D, variance_out[c] = lambda_c / (double)(n - 1); every one may be
 *               NULL; info->total_variance = (the sequential sum from +0 of S's diagonal in ascending d) / (double)(n - 1).
 * The result is a function of the matrix and d2 alone: never of launch shapes, of a tunable, of the handle or of the order in which
 * workgroups run; no float atomics; bitwise identical between calls and handles.  Like every evaluation call it works on the matrix as
 * f2v_get_embeddings would return it (pending minibatches are committed first), runs on the handle's stream and changes neither the
 * matrices nor the rand() stream nor any later training result; on a handle attached to a push exchange it reads this rank's replica.
 * Workspace, allocated on first use (grown on demand) and freed by f2v_destroy: ceil(n / 4096) x D (D + 1) / 2 doubles of piece chains
 * (the largest: 269 MB at n = 1 Mi, D = 512), D (D + 1) / 2 + D + d2 x D doubles and n x d2 floats.  The eigenproblem is the host's, O(D^3) per
 * sweep and not part of `seconds`.  seconds: device time between events around the call's own launches.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for a null info, d2 = 0, d2 > D, n < 2. */
#define F2V_PCA_PIECE 4096
typedef struct {
    double total_variance, seconds;
    uint32_t sweeps, converged;
} f2v_pca_t;
F2V_API int f2v_pca(f2v_handle h, uint32_t d2, float *y_out /* n x d2, may be NULL */, double *components_out /* d2 x D, may be NULL */,
            double *mean_out /* D, may be NULL */, double *variance_out /* d2, may be NULL */, f2v_pca_t *info);
/* f2v_trustworthiness -- neighbourhood preservation between the handle's matrix X and a second matrix Y (n x d2 on the host: the PCA
 * layout, a -dim 2 run, a t-SNE made elsewhere, yesterday's checkpoint).  For a matrix M and a vertex i, the order of M around i is the
 * result order of f2v_nearest_rows with F2V_SIM_L2 and F2V_NEAREST_EXCLUDE_SELF (the fp32 fma chain of squared differences, ascending
 * distance, -0 = +0, equal distances by ascending vertex id, a NaN after every number); r_M(i, j) is the 1-based place of j in it,
 * N_M(i, k) its first k vertices.  Then
 *   penalty_x(i) = sum over j in N_Y(i, k) of max(0, r_X(i, j) - k)    the neighbours the picture invents,
 *   penalty_y(i) = sum over j in N_X(i, k) of max(0, r_Y(i, j) - k)    the neighbours it loses,
 *   overlap(i)   = |N_X(i, k) n N_Y(i, k)|,
 * integers all three, their sums over the samples exact (penalty_x, penalty_y, hits: integer atomics, as in f2v_modularity), and the host
 * forms trustworthiness = 1.0 - (double)penalty_x * (2.0 / ((double)nq * k * (2.0 * n - 3.0 * k - 1.0))), continuity the same from
 * penalty_y, overlap = (double)hits / ((double)nq * k).  With every vertex a sample (sample_ids NULL) that is scikit-learn's
 * trustworthiness(X, Y, n_neighbors = k) term for term, and continuity is trustworthiness(Y, X).  A sample subset is ranked against ALL
 * n vertices; duplicate sample ids are legal.  Results are a function of (X, Y, k, samples) alone: never of "trust_chunk" (samples per
 * launch, default 8192), "trust_block" (sample rows per workgroup, 0 = 64 | 64 | 128; 128 holds where k <= 32), the "nearest_*" tunables,
 * the handle or the order in which workgroups run.  Evaluation rules as for f2v_pca.  Cost: every sample against all n rows in D and in
 * d2 dimensions, O(nq n D).  Workspace, allocated on first use and freed by f2v_destroy: Y (n x d2 floats), the nearest-neighbour
 * workspace, per sample of a chunk 2 k words of neighbour ids, k keys and k counts, per sample 5 words.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for a null Y or out, d2 = 0 or d2 > F2V_TRUST_MAX_DIM, k = 0, k > F2V_NEAREST_MAX_K or
 * 2 k >= n (scikit-learn's condition), a sample id >= n, nq = 0 together with sample_ids. */
#define F2V_TRUST_MAX_DIM 512
typedef struct {
    double trustworthiness, continuity, overlap, seconds;
    uint64_t penalty_x, penalty_y, hits;
} f2v_trust_t;
F2V_API int f2v_trustworthiness(f2v_handle h, const float *Y /* n x d2 */, uint32_t d2, uint32_t k, const uint32_t *sample_ids /* NULL: every vertex */,
                        uint32_t nq, uint64_t *penalty_x_out /* per sample, may be NULL */, uint64_t *penalty_y_out /* per sample, may be NULL */,
                        f2v_trust_t *out);

/* ---- t-SNE layout ---------------------------------------------------------------------------------------------------------------
 * The picture performancescores/runvisualization.py itself draws (:15, :177-181): exact t-SNE (van der Maaten and Hinton 2008, as
 * scikit-learn runs it with init = "pca") over a sparse neighbour affinity matrix, every order of summation fixed.  The result is a
 * function of (X, samples, parameters, P or y_init where given) alone: never of a tunable ("tsne_rows", rows per workgroup of the pair
 * kernel, 0 = automatic | 64 | 128 | 256; "tsne_slices", spans per workgroup of it, 0 = one; the "nearest_*" tunables), of launch
 * shapes, of the handle or of the order in which workgroups run; no float atomics, no in-grid waits.
 *
 *   points      the laid-out points are rows sample_ids[0 .. m) of X in that order (NULL: every vertex, m = n); everything below
 *               speaks of positions 0 .. m-1.  A subset is laid out exactly as a handle holding only those rows would be.
 *   neighbours  k = floor(3 * perplexity); N(i) is the result order of f2v_nearest_rows with F2V_SIM_L2 and F2V_NEAREST_EXCLUDE_SELF
 *               over the m points alone; d_ij = the negated score (the fp32 fma chain of squared differences), converted exactly to fp64.
 *   conditional affinities (scikit-learn's _binary_search_perplexity, all fp64)   per point beta = 1, lo = -inf, hi = +inf; one
 *               evaluation: p_j = exp(-beta * d_ij), S = sum p_j and T = sum d_ij * p_j over N(i) in result order, each from +0; S == 0: S =
 *               1e-8; H = log(S) + (beta * T) / S; diff = H - log(perplexity).  |diff| <= 1e-5 or the 100th evaluation ends the search; else
 *               diff > 0: lo = beta, beta = hi infinite ? beta * 2 : (beta + hi) / 2; otherwise hi = beta, beta = lo infinite ? beta / 2 :
 *               (beta + lo) / 2.  p_(j|i) = p_j / S of the last evaluation.  exp and log are the device library's: this is the one place
 *               where a host restatement agrees to a tolerance and not bit for bit -- which is why f2v_tsne accepts P.
 *   P           p_ij = (p_(j|i) + p_(i|j)) / (2.0 * m) for every pair where either term exists (an absent term is +0); an entry below the
 *               smallest normal double is dropped; a CSR whose column ids ascend inside a row.  (Host code, built without contraction.)
 *   start       without y_init: y_ic = (double)(the f2v_pca projection of the handle's WHOLE matrix, d2 components, at row sample_ids[i],
 *               component c) * (1e-4 / sqrt(variance_out[0] of that call)) -- scikit-learn's init = "pca" scaling, sqrt correctly rounded;
 *               update = 0, gains = 1.
 *   state       Y, update and gains are m x d2 doubles; pair arithmetic reads yf = (float)y.
 *   pair(i, j)  t_d = yf_id - yf_jd, a = (t_0 * t_0 + t_1 * t_1) [+ t_2 * t_2], w = 1.0f / (1.0f + a): every product, sum and the
 *               division one correctly rounded fp32 operation, no contraction.
 *   repulsion   the columns j = 0 .. m-1 are cut into pieces of F2V_TSNE_PIECE consecutive ids, the pieces grouped into spans of
 *               F2V_TSNE_SPAN pieces.  A piece is summed in fp32 from +0 in ascending j, j == i left out: z += w, r_d += (w * w) * t_d
 *               (rounded products); the piece sums are converted to fp64 and added sequentially from +0 inside their span; the span sums
 *               are added sequentially from +0 in ascending order: Z_i and R_id.  Z = the Z_i summed in pieces of 64 consecutive rows,
 *               each from +0, the piece sums added sequentially from +0.
 *   attraction  fp64, over the nonzeros of row i of P in column order in pieces of 64 entries, each piece from +0, the pieces added
 *               sequentially from +0: A_id += ((ex * p_ij) * (double)w) * (double)t_d; ex = exaggeration in iterations (0-based) below
 *               exaggeration_iters and 1.0 from there on.
 *   step        (scikit-learn's _gradient_descent; fp64, one rounded operation each) g = 4.0 * (A_id - R_id / Z); update * g < 0: gains
 *               += 0.2, otherwise gains *= 0.8; gains = max(gains, 0.01); g *= gains; update = momentum * update - lr * g; y += update.
 *               momentum = 0.5 in iterations below exaggeration_iters and 0.8 from there on; learning_rate 0: lr = max((double)m /
 *               exaggeration / 4.0, 50.0).  Exactly `iters` iterations: there is no early stop.
 *   KL          = the sum over the nonzeros of p_ij * (flog(p_ij) - (flog((double)w) - flog(Z))) with P unexaggerated, flog the logarithm
 *               of "exact all-pairs Force2Vec" above, w and Z those of the Y the sum is asked for; a row's entries in pieces of 64 as in
 *               the attraction, the row sums in pieces of 64 rows as in Z.  Evaluated after the last iteration (info->kl, info->z) and
 *               after every kl_every-th (f2v_tsne_kl_log, 1-based iteration numbers).  A pair with a = inf has w = 0, outside flog's
 *               domain: flog takes its steps on the bits of 0.0 all the same (k = -1023, m = 1) and returns -709.0895657128241, a
 *               finite term.
 *
 * f2v_tsne_affinities returns P: rowptr_out m + 1 words, colids_out and values_out `cap` entries (2 m k always suffice); *nnz_out
 * answers also where cap is too small (F2V_EINVAL then).  f2v_tsne runs the iteration from P -- the caller's (all three arrays; its
 * values positive normal doubles) or, with all three NULL, the one f2v_tsne_affinities would return -- and from y_init (m x d2 doubles)
 * or the PCA start, and writes y_out = (float)Y, m x d2.  Zeros in f2v_tsne_params select the defaults: perplexity 30, iters 1000,
 * exaggeration 12, exaggeration_iters 250, learning_rate automatic, kl_every never; params NULL: all defaults.  A P that is given
 * makes perplexity unused.
 * Evaluation rules as for f2v_pca: pending minibatches are committed first, the calls run on the handle's stream (plain launches, no
 * host synchronisation inside the iteration loop) and change neither the matrices nor the rand() stream nor any later training result; on
 * an attached handle they read this rank's replica.  Workspace, allocated on first use (grown on demand) and freed by f2v_destroy:
 * the m gathered rows, the nearest-neighbour workspace, m k ids, scores and conditionals, P, 3 m d2 doubles and 2 m d2 floats of state
 * and m x ceil(m / 1024) x (d2 + 1) doubles of span sums (the largest: 402 MB at m = 131072, d2 = 2).  Cost: m^2 pairs per iteration.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for a null output, d2 not 2 or 3 (or, for the PCA start, above D), m < 8, a sample id
 * >= n or a duplicate sample id, perplexity <= 1 or NaN, k = floor(3 * perplexity) > F2V_NEAREST_MAX_K or >= m, a negative or NaN
 * parameter, a P given in part, a P whose row pointers do not start at 0 and ascend, whose column ids do not ascend inside a row or
 * reach m or whose values are not positive normal numbers, a PCA start on a matrix whose first component has variance 0, cap too small. */
#define F2V_TSNE_PIECE 64
#define F2V_TSNE_SPAN 16
typedef struct {
    double perplexity, exaggeration, learning_rate;
    uint32_t iters, exaggeration_iters, kl_every, reserved;
} f2v_tsne_params;
typedef struct {
    double kl, z, learning_rate, seconds;  /* kl, z: of the final Y; learning_rate: the one used; seconds: device time of the iteration loop */
    uint64_t nnz;
    uint32_t k, reserved;  /* k: 0 where P was given */
} f2v_tsne_t;
F2V_API int f2v_tsne_affinities(f2v_handle h, const uint32_t *sample_ids /* NULL: every vertex */, uint32_t m, double perplexity,
                        uint32_t *rowptr_out /* m + 1 */, uint32_t *colids_out, double *values_out, uint64_t cap, uint64_t *nnz_out,
                        double *seconds_out /* may be NULL */);
F2V_API int f2v_tsne(f2v_handle h, const uint32_t *sample_ids /* NULL: every vertex */, uint32_t m, uint32_t d2, const f2v_tsne_params *params /* may be NULL */,
             const uint32_t *p_rowptr, const uint32_t *p_colids, const double *p_values /* all NULL: computed as above */,
             const double *y_init /* m x d2, or NULL: the PCA start */, float *y_out /* m x d2 */, f2v_tsne_t *info);
/* The last f2v_tsne's "kl_every" log: iterations_out (1-based) and values_out receive up to `cap` entries, *count_out the number logged
 * (both arrays may be NULL with cap = 0: count only). */
F2V_API int f2v_tsne_kl_log(f2v_handle h, uint32_t *iterations_out, double *values_out, uint32_t cap, uint32_t *count_out);

/* ---- fold-in---------------------------------------------------------------------------------------------------------------
 * What is the vector of a vertex that was not in the graph when it was trained?  A new vertex whose neighbours are all existing
 * vertices is a row whose update reads only frozen rows, so the training rule itself answers: f2v_fold_in runs `iters` epochs of the
 * step kernels' row update for each of m new vertices against the matrix X as it stands, every other row held fixed.  New vertices do
 * not see each other, so each is independent of the others and all its epochs run inside one launch.  The result is a function of
 * (X, the lists, option, iters, ns, lr, init, seed, index_base) alone: bitwise identical between calls, handles and GPUs and under
 * every tunable; no float atomics, no in-grid waits.  Every operation below is one rounded fp32 operation unless it says fp64.
 *   matrix      X as f2v_get_embeddings would return it (pending minibatches are committed first); the call runs on the handle's stream
 *               and changes neither the matrices nor the rand() stream nor any later training result; on a handle attached to a push
 *               exchange it reads this rank's replica;
 *   lists       vertex q of the call has the neighbours q_colids[q_rowptr[q] .. q_rowptr[q + 1]), ids of the n existing vertices, in the
 *               caller's order -- the summation order --, duplicates kept, deg(q) counting them; an empty list is legal.  Q = index_base
 *               + q is the vertex's index for every random draw: a call cut into several calls with matching index_base gives the
 *               same bits;
 *   pair(y, j)  the pair sum a over t_d (below) in the engine's per-pair order: the balanced adjacent-pair tree over next_pow2(D)
 *               zero-padded terms of the step kernels (ORC_ORDER_TREE of the test oracle);
 *   scale(v)    max(v, -5) then min(., 5), a NaN becoming -5;
 *   negatives   s(Q, e, k) = mix64(mix64(seed) ^ ((Q * iters + e) * ns + k)) % n for k = 0 .. ns-1, mix64 the splitmix64 finaliser of
 *               the objective above, 64-bit wrapping arithmetic: computed in the kernel, nothing is uploaded and nothing is drawn from
 *               the handle's stream; self-samples cannot occur (the vertex is not among the n);
 *   epoch       y^(e+1) from y = y^e, e = 0 .. iters-1: what the step kernels compute for a row whose pre-batch value is y, whose CSR
 *               row is the list, with "hub_chunk" = 0 (one sequential pass in list order) and the negatives s(Q, e, .), at the call's lr:
 *     t-distribution options (5, 8, 11; sample/algorithms.cpp:588-639): F from +0; for every list entry j in order t_d = y_d - x_jd,
 *               a = the pair sum of t_d * t_d, d1 = (float)(-2.0 / (1.0 + (double)a)) (fp64, narrowed), F_d = F_d + lr * scale(t_d * d1);
 *               then for every negative j = s(Q, e, k) in order the same with d1 = (float)(2.0 / ((double)a * (1.0 + (double)a)));
 *               y^(e+1)_d = y_d + F_d;
 *     sigmoid options (6, 9; :833-921): degi = (float)(1.0 / (double)(deg(q) + 1)), c0 = (double)(lr * degi); P = y; for every list
 *               entry j in order a = the pair sum of y_d * x_jd, sm = the 2048-entry table's sigmoid of a (f2v_sm_table; 1 above 6, 0
 *               below -6), coef = (1.0 - (double)sm) * c0 (fp64), P_d = (float)((double)x_jd * coef + (double)P_d); then for every
 *               negative in order w = lr * sm, P_d = P_d - w * x_jd; y^(e+1) = P.  (Both are `oracle.row` of the test oracle with
 *               ORDER_TREE and chunk 0 on the graph with the vertex appended as row n.)
 *               Every other option (1, 2-4, 7, 10) is F2V_EINVAL: walks for a vertex outside the CSR are out of scope;
 *   initial     F2V_FOLD_INIT_GIVEN: the caller's rows.  F2V_FOLD_INIT_RANDOM: y_d = v for the sigmoid options, 2v - 1 for the t options,
 *               v = (mix64(mix64(seed) ^ (2^63 | (Q * D + d))) >> 40) * 2^-24 (both exact in fp32).  F2V_FOLD_INIT_MEAN (the default):
 *               y_d = (float)(S_d / (double)deg), S_d the sequential fp64 sum from +0 of (double)x_jd in list order; a vertex with an
 *               empty list gets the RANDOM rule.  iters = 0 returns the initial vectors.
 *               (Why the mean: cora, option 5, one tenth of the vertices held out and folded in for 600 epochs, classified by a model
 *               fitted on the others: 0.83 from the mean, 0.76 from a random start, 0.87 trained jointly.  Under option 6 a random
 *               start reaches 0.25 only -- the sigmoid attraction is divided by deg + 1 and moves a vector slowly -- where the mean
 *               start gives 0.59 and the mean alone, iters = 0, 0.76 in the CPU experiment: DESIGN.md section 15.)
 * Launches: the vertices run in chunks of "fold_chunk" (default 65536), per chunk one kernel for the initial vectors (MEAN, RANDOM) and
 * one or two for the epochs, a chunk's vertices placed by descending list length (placement only).  Where D is a multiple of 4 up to
 * 256 and "quarter_wave" is on, a vertex is a quarter-wave of the step kernels' layout, else a wavefront; all epochs run inside the
 * launch with the vector in registers, the list's rows gathered four (a wavefront: eight) at a time and read again through the caches
 * every epoch.  "fold_resident" (-1 = automatic, the default | 0; both select that form): a resident form, which staged a workgroup's
 * list rows once in LDS and reread them there, was built and measured 7-11 % slower where it applies (DESIGN.md section 15,
 * profiles/foldin_time.txt); it is not part of the library, 1 is F2V_EINVAL and info->resident is always 0.  A vertex's epochs and
 * list entries are one sequential chain (about 0.25 us per entry and epoch at D = 128): a call lasts at least as long as its longest
 * list.  info->pairs: the (vertex, other row) interactions evaluated,
 * sum over q of (deg(q) + ns) * iters; info->seconds: device time between events around the call's own launches.  Workspace,
 * allocated on first use (grown for a larger call) and freed by f2v_destroy: the lists (m + 1 offsets, the ids), m words of
 * placement, and two chunk x D float matrices (initial vectors, results).
 * m = 0 is F2V_OK and touches nothing.  F2V_ESTATE without valid embeddings; F2V_EINVAL for a null pointer, an option that does not
 * fold in, a list id >= n, a descending q_rowptr, an unknown init_kind, GIVEN without init, n < 1, and where (index_base + m) * iters *
 * ns would reach 2^62.
 * Making folded vertices permanent: build a new engine on the grown CSR and f2v_set_embeddings the concatenated matrix; growing a live
 * handle's graph is out of scope. */
#define F2V_FOLD_INIT_MEAN 0   /* default */
#define F2V_FOLD_INIT_RANDOM 1
#define F2V_FOLD_INIT_GIVEN 2  /* `init` holds m x D floats */
typedef struct {
    double seconds;
    uint64_t pairs;
    uint32_t resident, reserved;
} f2v_fold_t;
F2V_API int f2v_fold_in(f2v_handle h, int option, const uint32_t *q_rowptr /* m + 1 */, const uint32_t *q_colids /* ids < n */, uint32_t m,
                uint32_t iters, uint32_t ns, float lr, int init_kind, const float *init /* m x D or NULL */, uint64_t seed, uint64_t index_base,
                float *y_out /* m x D */, f2v_fold_t *info /* may be NULL */);

/* ---- link prediction pairs ----------------------------------------------------------------------------------------------------
 * The pair set that the reference's link-prediction score is computed on (makeLinkPredictionData, performancescores/
 * runlinkpredict.py:51-107): every edge once as a positive, `ratio` times as many non-neighbours per vertex as negatives, shuffled;
 * f2v_logreg_fit on the first int(M * frac) pairs and f2v_logreg_decision on the others is the score.  The set is a function of (the
 * CSR, ratio, seed) alone: bitwise identical between calls, handles and GPUs and under every tunable; no float is involved.
 *   graph       N(u) = the distinct ids of CSR row u other than u itself: duplicates collapse, a self-loop is dropped.  Rows must be
 *               ascending (checked once per handle).  The call needs no embeddings; it runs on the handle's stream and touches neither
 *               the matrices nor the rand() stream nor any later result;
 *   positives   for u ascending, the v in N(u) with v > u, ascending; p(u) is their number.  On the symmetric CSRs of f2v_read_mtx
 *               that is every undirected edge once; a nonzero stored in one direction only counts where its row names it: (u, v)
 *               with v > u present in row u alone is a positive, present in row v alone it is none (and v is no neighbour of u);
 *   how many    A(u) = n - 1 - |N(u)|, total(u) = min(ratio * p(u), A(u) / 2) negatives, integer division; 1 <= ratio <= 16, the
 *               default everywhere is 2.  This is the reference's rule (:76-80) with its dense-vertex case -- (n - |N(u)|) / 2 for a
 *               vertex with more than n / 2 neighbours -- turned into a cap: the reference's loop does not end for a vertex of degree
 *               n / 2 whose neighbours are all higher; under the cap at least half of the admissible vertices stay free, a candidate
 *               is accepted with probability above A(u) / (2 n), and the expected number of candidates per vertex is below n.
 *               `capped` counts the vertices with A(u) / 2 < ratio * p(u);
 *   which       S1 = mix64(seed) (mix64: the splitmix64 finaliser of the objective above, 64-bit wrapping arithmetic); candidate
 *               c(u, t) = mix64(mix64(S1 ^ u) + t) % n for t = 0, 1, 2, ...; a candidate is accepted if it is not u, is not in N(u)
 *               and equals no earlier accepted candidate of u; u's negatives are its first total(u) accepted candidates, in order of
 *               t.  (The reference admits u itself as a negative; this definition does not.)  `candidates` = the sum over the
 *               vertices with total(u) > 0 of (the t of u's last accepted candidate + 1);
 *   order       item index i runs over u ascending: u's positives, then u's negatives in acceptance order; M = sum p(u) + sum total(u);
 *   shuffle     a keyed bijection, not a sort.  b = the smallest even number >= 2 with 2^b >= M, half = b / 2, mask = 2^half - 1,
 *               S2 = mix64(S1).  perm(i): x = i; repeat { L = x >> half, R = x & mask; for r = 0 .. 3: (L, R) = (R, L ^ (mix64(S2 ^
 *               (r * 2^32 + R)) & mask)); x = (L << half) | R } until x < M.  (A four-round Feistel network is a bijection of [0, 2^b)
 *               for any round function; walking its cycle until the value is below M makes it one of [0, M), and 2^b < 4 M keeps
 *               the walk short.)  Item i = (u, v, y) is written to place perm(i) of u_out / v_out / y_out, y = 1 for a positive
 *               and 0 for a negative.  The reference's split is then "the first int(M * frac) places train".
 * Calling: with u_out, v_out and y_out all NULL only *count_out = M and info are filled (info->candidates stays 0: nothing is
 * drawn); with the three given, `cap` is the number of pairs each holds: cap < M is F2V_EINVAL with *count_out = M written.  M = 0 is
 * F2V_OK.  F2V_EINVAL also for a null handle or count_out, one or two of the three outputs, a ratio outside 1..16, rows that are
 * not ascending, and a vertex with more than 2^29 negatives.  info->seconds: device time between events around the call's own launches.
 * Launches: |N(u)|, p(u) and total(u) by one wavefront per row ("distinct" is "differs from its predecessor"), three launches of a
 * 64-bit exclusive prefix sum for the items' offsets, then the vertices that draw negatives in the order of descending total(u)
 * (placement only): a vertex with at most "link_short_max" (0..1024, default 256) negatives is one wavefront's, 64 candidates a round,
 * its accepted set a list in LDS; a longer one a workgroup's, its accepted set an open-addressing table: in LDS, 256 candidates a
 * round, up to 3072 negatives, and in the workspace, 1024 candidates a round, above.  Every item is stored straight to its place.  Neither "link_short_max" nor
 * the round widths change a bit of the result.
 * Workspace, allocated on first use (grown for a larger call) and freed by f2v_destroy: per vertex p(u), total(u) (4 bytes each) and
 * the offset (8), 8 bytes per 1024 vertices of the prefix sum, 4 per vertex that draws negatives (placement), M x 9 bytes of
 * results, and per vertex with more than 3072 negatives a table of 8 bytes x the smallest power of two >= 2 total(u) + 2048, plus 8
 * bytes for its position.  The pairs travel to the host (9 M bytes) and, as id lists of f2v_logreg_*, back. */
typedef struct {
    double seconds;            /* device time between events around the call's own launches */
    uint64_t positives, negatives;
    uint64_t candidates;       /* candidates drawn in all: sum over u of (index of u's last accepted candidate + 1) */
    uint64_t capped;           /* vertices whose negatives were limited by the cap */
} f2v_link_t;
F2V_API int f2v_link_pairs(f2v_handle h, uint32_t ratio, uint64_t seed, uint32_t *u_out, uint32_t *v_out, uint8_t *y_out /* all three NULL: count only */,
                   uint64_t cap, uint64_t *count_out, f2v_link_t *info /* may be NULL */);

/* ---- held-out link prediction ---------------------------------------------------------------------------------------------------
 * The pair set above is the reference's protocol: the embedding is trained on every edge and a classifier is then asked to recognise
 * those same edges.  The standard protocol hides a share of the edges, trains on the rest, ranks the hidden edges against non-edges
 * and reports threshold-free ROC-AUC and average precision.  Three calls: f2v_edge_split (integers only), f2v_pair_scores (the
 * embedding's own similarity of arbitrary pairs) and f2v_ranking (scores and 0/1 labels -> AUC, AP).  All run on the handle's stream
 * as plain launches without in-grid waits or float atomics and touch neither the matrices nor the rand() stream nor any later
 * training result.  N(u), A(u) and "rows must be ascending" are those of the link prediction pairs; mix64 as there.
 * S1 = mix64(seed), SE = mix64(S1 ^ 0x65646765), SN = mix64(S1 ^ 0x6e656773).
 *
 * f2v_edge_split: a function of (the CSR, frac, seed, ratio) alone; it needs no embeddings.
 *   candidate   for u != v: a = min(u, v), b = max(u, v), key(a, b) = mix64(SE ^ (a * 2^32 | b)); T = (uint64)(frac * 2^64) for 0 <= frac
 *               < 1 (the product is exact, the conversion truncates); {a, b} is a hold-out candidate iff key < T.  A hash of the pair,
 *               not a draw: both directions of an edge and every duplicate decide alike without talking to each other;
 *   anchor      anchor(u) = the v in N(u) of smallest key(u, v), ties to the lower v; none where N(u) is empty.  The edge {u,
 *               anchor(u)} is never held out, so every vertex that had a neighbour keeps at least one: no vertex is left without a
 *               training signal.  CONNECTIVITY IS NOT PROMISED: a component may fall apart.  The anchors save candidates, so the held
 *               share lies below frac (`protected_edges` counts them);
 *   held        {a, b} is held iff it is a candidate, b != anchor(a) and a != anchor(b).  On a symmetric CSR both directions decide
 *               alike; on a CSR that stores a nonzero in one direction only the rule is applied per nonzero as written;
 *   training    row u keeps, in order, every nonzero v with v == u or {u, v} not held: duplicates and self-loops stay.  rowptr_train
 *               u32[n + 1], colids_train;
 *   positives   for u ascending, the v in N(u) with v > u and {u, v} held, ascending; q(u) is their number, H the total;
 *   negatives   non-edges of the FULL graph: total'(u) = min(ratio * q(u), A(u) / 2), 0 <= ratio <= 16 (0 draws none); candidates
 *               c'(u, t) = mix64(mix64(SN ^ u) + t) % n, accepted by the rule of f2v_link_pairs (not u, not in N(u), not an earlier
 *               accepted candidate of u); order: u ascending, then acceptance order.  There is no shuffle: a ranking does not depend
 *               on input order.  `capped` counts the vertices with A(u) / 2 < ratio * q(u), `drawn` the candidates drawn.
 * Calling (as f2v_link_pairs): with the six output arrays all NULL only the three counts and info are filled (info->drawn stays 0);
 * with all six given the capacities are checked: one too small is F2V_EINVAL with the counts written.  F2V_EINVAL also for a null
 * handle or count pointer, frac outside [0, 1) or NaN, a ratio above 16, rows that are not ascending, some outputs but not all, and
 * a vertex with more than 2^29 negatives.
 * Launches: the anchors by one wavefront per row (a minimum over the row), the decisions and counts by one wavefront per row, the
 * 64-bit exclusive prefix sum of the link-pair code three times (kept nonzeros, held pairs, negatives), one fill launch that writes
 * each kept nonzero and each held pair to its place, and the negative-drawing launches of f2v_link_pairs with SN as their stream
 * constant and the identity as their shuffle; "link_short_max" places them as there and changes no bit.
 * Workspace of its own (no other call's buffers are used or resized), allocated on first use, grown for a larger call and freed by
 * f2v_destroy: per vertex 5 x 4 and 3 x 8 bytes, 8 bytes per 1024 vertices, 4 (n + 1 + train_nnz) + 8 H + 9 negatives bytes of
 * results, 4 bytes per vertex that draws negatives and the tables of f2v_link_pairs for the vertices with more than 3072.
 *
 * f2v_pair_scores: scores_out[i] = the similarity of the "nearest neighbours" section with q = row u_ids[i] and c = row v_ids[i]:
 * the fp32 fma chain from +0 over ascending d; for F2V_SIM_COSINE r_v = 0 for a zero row.  A score is therefore bit-equal to the
 * score f2v_nearest_rows reports for the same (query, id) and metric (as there, -0 is reported as +0 and every NaN as one NaN).  It
 * works on the matrix as f2v_get_embeddings would return it (pending minibatches are committed first).  Any D.  Pairs are uploaded
 * and run in chunks of "pairs_chunk" (f2v_set_param, 1 .. 2^26, default 2^20: 12 bytes of workspace a pair); the chunk size never
 * changes a bit.  One wavefront per 64 pairs: 32 dimensions of the 128 rows a round are loaded by the whole wavefront, coalesced,
 * into a padded LDS tile, then every lane runs its own pair's chain from LDS.  seconds_out (may be NULL): device time around the
 * launches.  F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers, an id >= n, an unknown metric.  m = 0 is F2V_OK and
 * touches nothing.
 *
 * f2v_ranking: scores double[m], y u8[m] (0 or 1), m < 2^31.  Larger scores rank first; -0 and +0 are one score; NaN ranks below
 * every number and all NaNs tie.  P and N are the counts of 1 and 0.  The groups of equal score are taken in descending order, g = 1
 * .. G, with pos_g ones and neg_g zeros:
 *   concordant = sum_g pos_g * (zeros in later groups), tied = sum_g pos_g * neg_g, both exact uint64;
 *   auc = (double)(2 * concordant + tied) / (2.0 * (double)P * (double)N), formed on the host: Mann-Whitney with half credit for
 *         ties (scikit-learn's roc_auc_score);
 *   ap  = sum / (double)P: TP_g, FP_g the inclusive cumulative ones and zeros through group g, term_g = ((double)pos_g * (double)TP_g)
 *         / (double)(TP_g + FP_g) sits at the sorted position of the group's last item (every other position holds +0); the positions
 *         are cut into blocks of 1024, a block is summed sequentially from +0, the block sums are added sequentially in ascending
 *         order (scikit-learn's average_precision_score).
 * The result is a function of the multiset of (score, label) alone -- permutation-invariant bit for bit -- and of no tunable.  Each
 * score becomes an order-preserving 64-bit key (-0 canonicalised, NaN the lowest), the keys are sorted with the labels as payload
 * (rocprim::radix_sort_pairs; the order inside a group is never looked at), then cumulative ones are scanned, every group's last item
 * finds the group's first by binary search and forms the tallies (integer atomics) and its term.  Workspace: 38 bytes per item plus
 * the sort's.  F2V_EINVAL for a label above 1, P = 0, N = 0 (out->positives / negatives are written), m >= 2^31, null pointers. */
typedef struct {
    double seconds;            /* device time between events around the call's own launches */
    uint64_t edges;            /* distinct undirected edges, self-loops left out */
    uint64_t candidates_held;  /* ... of them with key < T */
    uint64_t protected_edges;  /* candidates that an anchor saved */
    uint64_t held;             /* H = candidates_held - protected_edges */
    uint64_t train_nnz;
    uint64_t negatives;
    uint64_t drawn;            /* candidates drawn for the negatives */
    uint64_t capped;           /* vertices whose negatives were limited by the cap */
} f2v_split_t;
F2V_API int f2v_edge_split(f2v_handle h, double frac, uint64_t seed, uint32_t ratio, uint32_t *rowptr_train /* n + 1 */, uint32_t *colids_train,
                   uint64_t cap_train, uint32_t *held_u, uint32_t *held_v, uint64_t cap_held, uint32_t *neg_u, uint32_t *neg_v, uint64_t cap_neg,
                   uint64_t *train_nnz_out, uint64_t *held_out, uint64_t *negatives_out, f2v_split_t *info /* may be NULL */);
F2V_API int f2v_pair_scores(f2v_handle h, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, int metric, float *scores_out,
                    double *seconds_out);
typedef struct {
    double auc, ap;
    uint64_t concordant, tied;
    uint64_t positives, negatives;  /* P, N */
    uint64_t groups;                /* G */
    double seconds;                 /* device time between events around the call's own launches */
} f2v_ranking_t;
F2V_API int f2v_ranking(f2v_handle h, const double *scores, const uint8_t *y, uint64_t m, f2v_ranking_t *out);

/* ---- neighbourhood scores of pairs ------------------------------------------------------------------------------------------------
 * The yardstick of a held-out link prediction: the classic scores of a pair from the graph alone -- common neighbours, Jaccard,
 * Adamic-Adar, resource allocation, preferential attachment -- computed on the training graph's handle for the hidden edges and the
 * negatives and ranked by f2v_ranking like the embedding's own similarity.  The result is a function of (the CSR, the pair, kinds)
 * alone: bitwise identical between calls, handles and GPUs and under every tunable; no float atomics.
 *   graph       N(u) is that of the link prediction pairs: the distinct ids of CSR row u other than u itself; d(u) = |N(u)|.  Rows must
 *               be ascending (checked once per handle).  The call needs no embeddings; it runs on the handle's stream as plain launches
 *               without in-grid waits and touches neither the matrices nor pending minibatches nor the rand() stream nor any later
 *               training result;
 *   pair        any u, v < n; u == v is legal.  W(u, v) = N(u) n N(v), the common neighbours; no member of W is u or v;
 *   S and L     S = the one of u, v whose STORED row has fewer nonzeros (rowptr[x + 1] - rowptr[x]), ties to the lower vertex id; L =
 *               the other one; for u == v both are u.  S's stored row is cut into pieces of F2V_NB_PIECE = 1024 consecutive nonzeros:
 *               duplicates and a self-loop keep their places;
 *   kinds       bits, every value fp64, c = |W|:
 *               F2V_NB_COMMON        (double)c, exact;
 *               F2V_NB_JACCARD       (double)c / (double)(d(u) + d(v) - c), one rounded division; +0 where the denominator is 0;
 *               F2V_NB_ADAMIC_ADAR   the sum over w in W of 1.0 / flog((double)d(w)), flog that of the exact objective (option 1); a
 *                                    w with d(w) < 2 adds nothing (on a CSR that stores a nonzero in one direction only a common
 *                                    neighbour can have d(w) of 0 or 1);
 *               F2V_NB_RESOURCE      the sum over w in W of 1.0 / (double)d(w); a w with d(w) = 0 adds nothing;
 *               F2V_NB_PREFERENTIAL  (double)d(u) * (double)d(v), one rounded multiplication;
 *   order       of the two sums: a nonzero of S's stored row is a member of W iff it is the first of its run of equal ids, is
 *               neither u nor v, and is in L's row.  Inside a piece the members' terms are added sequentially from +0 in ascending
 *               position; the piece sums are added sequentially from +0 in ascending piece order.  A pair whose S row has at most 1024
 *               nonzeros is therefore one plain sequential sum;
 *   symmetry    every score of (u, v) equals that of (v, u) bit for bit: the choice of S is symmetric.
 * scores_out holds popcount(kinds) arrays of m doubles, kind-major, in ascending order of the kinds' bits: with kinds = JACCARD | RESOURCE
 * the Jaccard values are scores_out[0 .. m) and the resource-allocation values scores_out[m .. 2m).  seconds_out (may be NULL): device
 * time between events around the call's own launches.  F2V_EINVAL for null pointers, kinds == 0 or a bit above 16, an id >= n (checked
 * on the host before anything is uploaded: no kernel sees one) and rows that are not ascending.  m = 0 is F2V_OK and touches nothing.
 * The call works on a handle without embeddings: it never returns F2V_ESTATE.
 * Launches: d(u) for every vertex by one wavefront per row, once per handle, kept in n words of the handle's own.  Pairs are uploaded
 * and run in chunks of "pairs_chunk" (see f2v_pair_scores); the chunk size never changes a bit.  Per chunk: one thread per pair counts
 * the pair's pieces, the 64-bit exclusive prefix sum of the link-pair code gives the place of its first work item, one launch fills the
 * item list, then one wavefront per work item (grid stride; at most 8192 workgroups of four wavefronts) takes a piece of a pair with
 * several pieces, or a whole pair: 64 consecutive nonzeros of S's row a round, a lower-bound search of each lane's id in L's row (as
 * many steps as the row length has bits, at most 32), a ballot for the round's members, every member lane its own two terms, and the
 * terms added in ascending lane order, one cross-lane read per set bit.  A last launch, one thread per pair, adds the piece results
 * of the pairs with several pieces in ascending piece order.  Only F2V_NB_PREFERENTIAL asked for: nothing is searched.  Neither
 * Adamic-Adar nor resource allocation asked for: no term is formed.  "neighbourhood_spread" (f2v_set_param, default 1; 0: one wavefront
 * walks all pieces of its pair) is placement only; "last_neighbourhood_items" reads the piece items of the last call.
 * Workspace of its own (no other call's buffers are used or resized), allocated on first use, grown for a larger call and freed by
 * f2v_destroy: 4 n bytes of degrees; per pair of a chunk 16 bytes of ids and counts, 8 of offset and 8 per kind asked for; 8 bytes
 * per 1024 pairs of the prefix sum; 28 bytes per piece item. */
#define F2V_NB_PIECE 1024
#define F2V_NB_COMMON 1u
#define F2V_NB_JACCARD 2u
#define F2V_NB_ADAMIC_ADAR 4u
#define F2V_NB_RESOURCE 8u
#define F2V_NB_PREFERENTIAL 16u
#define F2V_NB_ALL 31u
F2V_API int f2v_pair_neighbourhood(f2v_handle h, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, uint32_t kinds,
                           double *scores_out /* popcount(kinds) arrays of m, kind-major, ascending bit */, double *seconds_out /* may be NULL */);

/* ---- ranks of pairs -----------------------------------------------------------------------------------------------------------------
 * For a hidden edge (u, v): where does v stand among ALL vertices when they are ordered by similarity to u, the edges already known
 * filtered out?  The answers over a set of pairs are the mean reciprocal rank, the mean rank and Hits@K.  The sampled negatives of
 * f2v_edge_split are mostly easy ones; a rank of 5000 among n says what an AUC against them cannot, and a top-k stops at
 * F2V_NEAREST_MAX_K.
 *   scores      for pair i let u = u_ids[i], v = v_ids[i].  For every vertex w, s_w is the similarity of "nearest neighbours" with q = row
 *               u and c = row w (the fp32 fma chain from +0 over ascending d; cosine with r = 0 for a zero row): bit-equal to
 *               f2v_pair_scores(u, w) and to the score f2v_nearest_rows reports.  t = s_v;
 *   order       W(s) = 0 for a NaN; otherwise, with b = bits(s + 0.0f), W = ~b where the sign bit is set, else b | 0x80000000.  w ranks
 *               above v iff W(s_w) > W(t) and ties with v iff W(s_w) == W(t): -0 and +0 are one score, a NaN is below every number, all
 *               NaNs tie -- the rules of f2v_nearest_* and f2v_ranking;
 *   filter      E(u, v) is the set of DISTINCT vertices made of {u} if F2V_NEAREST_EXCLUDE_SELF is set and of N(u), the CSR row of u in
 *               the handle's graph, if F2V_NEAREST_EXCLUDE_NEIGHBOURS is set (a duplicated nonzero counts once; a self-loop makes u a
 *               member once); v itself is then always removed from E: the target stays a target even where it is u or a neighbour of
 *               u in the handle's CSR.  The candidates are C = {0 .. n-1} \ E \ {v}.  On the training graph's handle with both flags
 *               set this is the "filtered" setting of the literature.  Only the edges that the handle's CSR knows are filtered: other
 *               hidden edges of u remain candidates;
 *   outputs     greater_out[i] = #{w in C : w ranks above v}; equal_out[i] = #{w in C : w ties with v}; rank2_i = 2 + 2 greater + equal,
 *               twice the mid-rank, an exact uint64 (ties count half, as in f2v_ranking); hits_out[j] = #{i : rank2_i <= 2 ks[j]}, nk <=
 *               F2V_RANKS_MAX_KS, every ks[j] >= 1;
 *   info        seconds (device time between events around the call's own launches), pairs = m, rank2_sum (uint64), mean_rank =
 *               (double)rank2_sum / (2.0 m), mrr = sum / (double)m -- the terms are 2.0 / (double)rank2_i in input order, blocks of 1024
 *               pairs are each summed sequentially from +0 and the block sums added sequentially in ascending order, on the host from
 *               the integers --, candidates = the sum of |C| over the pairs, tied_pairs = the pairs with equal > 0.
 * Guarantees.  The two integers of a pair are a function of (the matrix, the CSR, u, v, metric, flags) alone: never of which other pairs
 * share the call or of their order, of "ranks_chunk" (f2v_set_param: pairs per launch, default 8192) or "ranks_splits" (candidate ranges a
 * block of pairs is counted in, 0 = automatic .. 256), of the handle, or of the order in which workgroups or atomics land: the only
 * atomics are integer additions.  Where equal == 0, v is not excluded by the flags and greater < k, f2v_nearest_rows(u, k, metric,
 * flags) holds v at index `greater`.  The call works on the matrix as f2v_get_embeddings would return it (pending minibatches are
 * committed first), on the handle's stream, and touches neither the matrices nor the rand() stream nor any later training result.  On a
 * handle attached to a push exchange it reads this rank's replica.
 * Launches, per chunk of pairs, all plain: the targets by the kernel of f2v_pair_scores; the base counts over all n rows by a kernel of
 * the shape of the nearest-neighbour one (the chunk's u rows resident in LDS, candidate tiles of 128, dot and cosine on
 * v_mfma_f32_32x32x2_f32, L2 on the vector ALU) that compares where that one selects and keeps two counters per pair, no scores and
 * no keys; a correction, one wavefront per (pair, piece of 256 nonzeros of row u), that scores the members of E by the chain of
 * f2v_pair_scores and subtracts those that ranked above or tied -- and v itself, which ties with itself.  "last_ranks_base_us" and
 * "last_ranks_correct_us" read the device time of the last call's base and correction launches.
 * Workspace of its own, allocated on first use, grown for a larger call and freed by f2v_destroy: per pair of a chunk D + 5 words, 8
 * bytes per work item of the correction, n words of reciprocal norms for cosine.
 * F2V_ESTATE without valid embeddings; F2V_EINVAL for null pointers, an id >= n, an unknown metric or flag bit, nk > F2V_RANKS_MAX_KS, a
 * zero K and -- with F2V_NEAREST_EXCLUDE_NEIGHBOURS -- rows that are not ascending (checked once per handle).  m = 0 is F2V_OK and touches
 * nothing. */
#define F2V_RANKS_MAX_KS 16
typedef struct {
    double seconds;
    uint64_t pairs;
    uint64_t rank2_sum;
    double mean_rank, mrr;
    uint64_t candidates;
    uint64_t tied_pairs;
} f2v_pair_ranks_t;
F2V_API int f2v_pair_ranks(f2v_handle h, const uint32_t *u_ids, const uint32_t *v_ids, uint64_t m, int metric, uint32_t flags,
                   uint32_t *greater_out /* m */, uint32_t *equal_out /* m */, const uint32_t *ks /* nk, may be NULL with nk = 0 */, uint32_t nk,
                   uint64_t *hits_out /* nk */, f2v_pair_ranks_t *info /* may be NULL */);

/* ---- components and spanning forests ----------------------------------------------------------------------------------------------
 * What the graph is made of: its connected components, a spanning forest of them under a keyed order, a hold-out split that the forest
 * keeps connected, and the subgraph induced on a vertex set (the largest component, say).  All integers; every result is unique by its
 * definition, so it is the same bits under every launch shape, schedule and handle.  The calls need no embeddings and run on the
 * handle's stream as plain launches without in-grid waits or float atomics (integer atomics only: minima, maxima and sums, whose
 * results do not depend on their order); they touch neither the matrices nor pending minibatches nor the rand() stream nor any later
 * training result.
 *   graph       the simple undirected graph f2v_modularity uses: a pair {a < b} is an edge iff (a, b) or (b, a) occurs as a nonzero;
 *               duplicates collapse, self-loops are ignored.  A CSR that stores an edge in one direction only gives the answers of
 *               its symmetric form.  Rows must be ascending (the cached check of f2v_link_pairs; F2V_EINVAL otherwise).
 *
 * f2v_components: labels_out[v] = the smallest vertex id in v's component; sizes_out[v] (may be NULL) = the size of that component.
 *   info        components; isolated = the vertices with no neighbour but themselves (components of size 1); largest = the size of
 *               the largest component and largest_label its label, ties to the lowest label; edges = the distinct pairs; rounds =
 *               the hooking rounds run, the last of which found nothing to hook: with L(v) = v at first, a round takes P = L, lowers
 *               P[max(L(u), L(v))] to min(L(u), L(v)) for every nonzero (u, v) with L(u) != L(v) -- all of them against the L the
 *               round began with -- and sets L(v) = the root of v under P.  (L and P are minima, so `rounds` too is a function of the
 *               graph alone.)  seconds: device time between events around the call's own launches.
 *   Launches: per round one hook launch (a wavefront per row piece: rows longer than 256 nonzeros are cut into pieces of 256, each a
 *   wavefront's of its own; 32-bit atomicMin), pointer-jumping launches until every vertex names its root (a launch moves a vertex up
 *   to 16 steps; the host reads two words per launch) and a copy; then sizes by 32-bit atomic adds on the labels (one per distinct
 *   label among a wavefront's non-roots) and one launch of counts.  The distinct pairs: a nonzero that differs from its predecessor
 *   counts at its lower end, or at its upper end where the lower end's row does not hold it (binary search).  F2V_EINVAL: a null
 *   handle, labels_out or info, rows not ascending.
 *
 * f2v_spanning_forest: S1, SE and key(a, b) = mix64(SE ^ (a * 2^32 | b)) are those of f2v_edge_split for the same seed.  bits =
 * "forest_key_bits" (f2v_set_param, 1..64, default 64).  The order on the pairs is lexicographic on (key(a, b) >> (64 - bits), a, b):
 * strict and total.  "forest_key_bits" is a DIAGNOSTIC knob: small values force key ties so that the (a, b) tie-break decides; it
 * never affects which pairs are hold-out candidates.  greatest = 0: the least forest, Kruskal over the pairs in ascending order;
 * greatest = 1: the greatest forest, Kruskal in descending order.  Under a strict total order either is unique.  Output: the forest's
 * pairs with u_out[i] < v_out[i], ascending by (u, v); *count_out = n - components.  With u_out and v_out both NULL only the count and
 * info are written; with both given `cap` is what each holds: cap < count is F2V_EINVAL with *count_out written.  info: seconds,
 * edges (the distinct pairs), forest_edges (= count), components, rounds.  F2V_EINVAL also for a null handle or count_out, one of the
 * two outputs without the other, greatest > 1, rows not ascending.
 *   Launches: Boruvka.  A round: every component finds its best outgoing pair under the order in two steps, because key and pair
 *   together are 128 bits -- a wavefront per row piece (as above: hub rows do not serialise a round) reduces the shifted keys of the
 *   nonzeros whose other end lies in another component and adds its maximum to the component's word (64-bit atomicMax; the least
 *   forest maximises the complements), then, among the nonzeros that match the component's key, the packed pair the same way.  Where
 *   the CSR is not structurally symmetric (checked once per handle, as f2v_louvain does) every such nonzero also proposes itself to
 *   the other end's component, whose rows may not hold it.  Then every root that found a pair hooks to the root at the pair's other
 *   end and appends the pair to the forest; two roots that chose the same pair are a mutual choice, broken towards the lower root, so
 *   no cycle forms.  The labels are flattened by pointer jumping as above.  The loop ends with the round in which no component found
 *   an outgoing pair (`rounds` counts it); every round scans all nonzeros.  The pairs are sorted (rocprim::radix_sort_keys).
 *   f2v_forest_round_seconds: host wall time of each round of the handle's last forest (seconds_out may be NULL: the count only).
 *
 * f2v_edge_split_connected: the argument list, the f2v_split_t and the definition of f2v_edge_split but for the protection rule:
 *   held        {a, b} is held iff it is a candidate (key(a, b) < T: the full 64-bit key, whatever "forest_key_bits") and is not in
 *               the greatest forest of the same seed.  `protected_edges` counts the candidates the forest saved.  The forest is a
 *               property of the pair: both stored directions and every duplicate decide alike, on a one-directional CSR too.
 *   Negatives, the training CSR, the order of the results and the calling conventions are those of f2v_edge_split, with q(u) taken
 *   from the new held set; as there, positives are listed, and `edges` and the candidates counted, from the rows as stored (v in N(u),
 *   v > u).  THE TRAINING GRAPH HAS EXACTLY THE COMPONENTS OF THE FULL GRAPH: the forest spans every component and none of its pairs
 *   is held.  NO CONNECTIVITY-PRESERVING RULE HOLDS MORE CANDIDATES: with 64 bits the candidates are a lower set of the order (key < T),
 *   so Kruskal in descending order takes every non-candidate it can before the first candidate and uses a candidate only where no
 *   non-candidate joins the two parts: as few candidates as any spanning forest can contain, and a training graph that keeps the
 *   components must contain a spanning forest.  (f2v_edge_split, its anchors and its bits are unchanged.)
 *   Launches: the forest as above (kept per handle for the last seed and "forest_key_bits": a second call with them does not run it
 *   again), one launch that flags every nonzero whose pair is in the sorted forest (binary search: both stored directions and every
 *   duplicate), then the launches of f2v_edge_split without the anchor launch, the decisions reading the flag.
 *
 * f2v_subgraph: keep u8[n], nonzero = kept.  The induced subgraph on the kept vertices, relabelled by rank among them: ascending old
 * id gives ascending new id, so rows stay ascending; duplicates and self-loops are kept as stored.  rowptr_out u32[rows + 1] (rows =
 * the number of kept vertices: the caller knows it), colids_out of `cap` entries, new_id_out u32[n] (may be NULL): the new id of v, or
 * 0xFFFFFFFF where v is dropped.  *rows_out and *nnz_out are always written; with rowptr_out and colids_out both NULL nothing else is
 * (count only; new_id_out is then not written either); cap < nnz is F2V_EINVAL with the counts written.  F2V_EINVAL also for a null
 * handle, keep, rows_out or nnz_out, and one of the two arrays without the other.  Launches: a count (a wavefront per row), the 64-bit
 * exclusive prefix sum of the link-pair code twice (new ids, row starts), a fill.  "last_subgraph_us" (f2v_get_param): its device time.
 *
 * Workspace of its own (no other call's buffers are used or resized), allocated on first use, grown for a larger call and freed by
 * f2v_destroy: 12 bytes per piece of a row longer than 256 nonzeros; components 4 x 4 bytes per vertex; the forest 2 x 4 + 4 x 8 bytes
 * per vertex plus the sort's, and 1 byte per nonzero for the split's flags; the subgraph 1 + 4 x 4 + 2 x 8 bytes per vertex, 8 per
 * 1024 vertices and 4 (rows + 1 + nnz) of results. */
typedef struct {
    double seconds;          /* device time between events around the call's own launches */
    uint64_t edges;          /* distinct pairs */
    uint32_t components;
    uint32_t isolated;       /* vertices with no neighbour but themselves */
    uint32_t largest;        /* size of the largest component */
    uint32_t largest_label;  /* ... and its label, ties to the lowest */
    uint32_t rounds;
} f2v_components_t;
F2V_API int f2v_components(f2v_handle h, uint32_t *labels_out /* n */, uint32_t *sizes_out /* n, may be NULL */, f2v_components_t *info);
typedef struct {
    double seconds;
    uint64_t edges;          /* distinct pairs */
    uint64_t forest_edges;   /* n - components */
    uint32_t components;
    uint32_t rounds;
} f2v_forest_t;
F2V_API int f2v_spanning_forest(f2v_handle h, uint64_t seed, uint32_t greatest /* 0 | 1 */, uint32_t *u_out, uint32_t *v_out /* both NULL: count only */,
                        uint64_t cap, uint64_t *count_out, f2v_forest_t *info /* may be NULL */);
F2V_API int f2v_forest_round_seconds(f2v_handle h, double *seconds_out /* may be NULL */, uint32_t cap, uint32_t *count_out);
F2V_API int f2v_edge_split_connected(f2v_handle h, double frac, uint64_t seed, uint32_t ratio, uint32_t *rowptr_train /* n + 1 */, uint32_t *colids_train,
                             uint64_t cap_train, uint32_t *held_u, uint32_t *held_v, uint64_t cap_held, uint32_t *neg_u, uint32_t *neg_v,
                             uint64_t cap_neg, uint64_t *train_nnz_out, uint64_t *held_out, uint64_t *negatives_out, f2v_split_t *info /* may be NULL */);
F2V_API int f2v_subgraph(f2v_handle h, const uint8_t *keep /* n */, uint32_t *rowptr_out /* rows + 1 */, uint32_t *colids_out /* both NULL: count only */,
                 uint64_t cap, uint32_t *new_id_out /* n, may be NULL */, uint32_t *rows_out, uint64_t *nnz_out);

/* ---- communities ----------------------------------------------------------------------------------------------------------------
 * What the graph itself achieves, to hold the modularity of an embedding's clusters against: the reference colours its pictures by
 * the graph's communities and prints their modularity (performancescores/runvisualization.py:127-152) and sweeps k-means for the best
 * modularity (runnodeclassclust.py:311-331).  f2v_louvain is the Louvain method in a form that is parallel and exact at once: every
 * quantity is an integer until the final Q, so the result is a function of (CSR, seed, max_levels, max_sweeps) alone -- never of
 * launch shapes, tunables, handles, the order in which workgroups or lanes run, or the order in which a coarse row stores its columns.
 *   graph       the simple undirected graph f2v_modularity uses: a pair u != v that occurs as a nonzero is one edge of weight 1
 *               (duplicates collapse), a diagonal nonzero is a self-loop: one edge, adding 2 to its vertex's degree.  Rows must be
 *               ascending (checked once per handle) and the CSR structurally symmetric: every nonzero (u, v), u != v, has (v, u)
 *               (checked once per handle on the device, by binary search in row v); 2m, the sum of the degrees, must be below 2^31:
 *               every product below then fits a signed 64-bit integer;
 *   level       a weighted graph with nodes 0 .. N_l - 1, integer weights w(i, j) = w(j, i) > 0 for i != j, loop(i) the weight of the
 *               edges inside node i, k(i) = sum_j w(i, j) + 2 loop(i); 2m is the same at every level.  Level 0 is the graph above
 *               with loop = 1 for a vertex that has a self-loop;
 *   moving      start with c(i) = i, tot(c) = k(c), size(c) = 1.  class(i) = mix64(mix64(seed + l) ^ i) % F2V_LOUVAIN_PHASES (mix64: the
 *               splitmix64 finaliser of the objective's section, seed + l wraps in 64 bits, l the level index).  A sweep is 8
 *               sub-rounds p = 0 .. 7; in sub-round p every node of class p with at least one neighbour j != i decides, all of them
 *               from the state (c, tot, size) as it was when the sub-round began: a = c(i); for every community d that holds a
 *               neighbour j != i, e(d) = the sum of w(i, j) over those j (e(a) = 0 if a holds none); tot'(d) = tot(d) - k(i) if d == a,
 *               else tot(d); score(d) = e(d) * 2m - k(i) * tot'(d) in signed 64-bit; best = the adjacent community of largest score,
 *               ties to the lowest id (a is adjacent only if it holds a neighbour); i moves to best iff best != a and score(best) >
 *               score(a) strictly -- except that it stays when size(a) == 1, size(best) == 1 and best > a: two singletons never
 *               swap.  After the decisions the moves are applied and tot and size updated (integer sums: order-free);
 *   level end   after every sweep Qnum = sum_c (in2(c) * 2m - tot(c)^2), in2(c) the sum of w(i, j) over the ordered pairs i != j
 *               inside c plus 2 loop(i) over its members (two sums of at most 2^62, formed separately and subtracted).  start =
 *               Qnum of the singleton state, best = the largest so far (at first start).  A sweep whose Qnum exceeds best becomes
 *               best and its labelling is kept, and the next sweep runs unless max_sweeps have run; otherwise the level ends with the
 *               kept labelling.  A level never lowers Qnum;
 *   aggregation the kept communities are renumbered 0 .. K - 1 in ascending id; node C of the next level has loop(C) = its members'
 *               loops + the weights of the edges between its members (each unordered pair once), w(C, D) = the sum of w(i, j) across
 *               the two; a vertex's label becomes the renumbered community of its node;
 *   stop        after a level whose best == start (an identity, still applied and recorded), or after max_levels levels.
 * Results: labels_out[v] in 0 .. communities - 1; level_labels_out[l * n + v] the label of v after level l; one record per level --
 * nodes, communities, sweeps (those run, the rejected last one included), moves (summed over them), qnum (the level's best); info:
 * communities, levels, edges (= m), seconds, and modularity = exactly what f2v_modularity returns for labels_out (the same tallies,
 * the same host formula).  The call needs no embeddings; it runs on the handle's stream and touches neither the matrices nor the
 * rand() stream nor any later training result.  Defaults everywhere: seed 1, max_levels 32, max_sweeps 64.  F2V_EINVAL: a null handle,
 * labels_out or info_out, a zero maximum, rows not ascending, an asymmetric CSR, 2m >= 2^31.
 * Launches: a unit's (a node's when moving, a community's when aggregating) weights to the communities around it are summed in an
 * open-addressing table of (community, weight) -- integer compare-and-swap on keys, integer adds on weights, a power of two of slots,
 * at least twice the nonzeros of the unit's rows, every probe loop bounded by the slots.  Units whose rows hold at most
 * "louvain_short_max" (0..256, default 32) nonzeros take 16 lanes each, sixteen to a workgroup, tables in LDS; longer ones a workgroup
 * each, the table in LDS up to "louvain_lds_slots" (0..8192, default 4096) slots and in the workspace above.  Decisions go to a
 * per-node array; a second launch applies them.  Neither tunable changes a bit.  The host reads back 24 bytes per sweep.
 * Workspace, allocated on first use (grown for a larger call) and freed by f2v_destroy: 4 bytes x 11 per vertex, per level node 8
 * bytes of placement, two sets of coarse graphs (per node 16 bytes, per nonzero of the finer level 8), 8 bytes per table slot of the
 * units above "louvain_lds_slots" of one sub-round, 4 bytes per 1024 nodes of the prefix sums, 1 KiB of counters.
 *
 * f2v_partition_agreement: how far two labellings agree.  a and b hold n labels each, below ka / kb, or F2V_LABEL_NONE (the vertex
 * takes no part).  N counts the vertices labelled in both; n_ij is the contingency table with row sums a_i and column sums b_j, counted
 * on the device with integer atomics; ka * kb <= F2V_AGREEMENT_MAX_CELLS.  Integers: n = N, sum_comb = sum_ij C(n_ij, 2), sum_a =
 * sum_i C(a_i, 2), sum_b = sum_j C(b_j, 2), total = C(N, 2), rows / cols = the non-empty rows and columns.  Floats, all fp64: S_ab =
 * the sum of n_ij * flog(n_ij) over the nonzero cells in row-major order, in pieces of 1024 consecutive cells -- each piece summed from
 * +0 in order, the piece sums added in order from +0 (flog: the logarithm of the option-1 objective) --, S_a and S_b likewise over the
 * row and column sums; H(A) = flog(N) - S_a / N, H(B) likewise, and exactly 0 for a side with one non-empty class (rows == 1, cols == 1:
 * decided on the integers, the rounded difference is not 0 for every N); mi = max(0, (S_ab - S_a - S_b) / N + flog(N)), and exactly 0
 * where either side has one non-empty class; nmi = mi / (0.5 * (H(A) + H(B))), 1 where both entropies are 0; ari = (sum_comb - sum_a * sum_b / total) / (0.5 * (sum_a + sum_b) - sum_a * sum_b /
 * total) on the fp64 conversions of the integers, 1 where the denominator is 0.  Bit-reproducible from the inputs.  F2V_EINVAL: null
 * arguments, ka or kb zero, too many cells, a label that is neither below its bound nor F2V_LABEL_NONE, N < 2.
 * Workspace: 8 bytes per vertex, 4 per cell, row and column, 8 per 1024 of them. */
#define F2V_LOUVAIN_PHASES 8
#define F2V_AGREEMENT_MAX_CELLS (1u << 26)
typedef struct {
    uint32_t nodes, communities, sweeps, reserved;
    uint64_t moves;
    int64_t qnum;
} f2v_louvain_level_t;
typedef struct {
    double modularity, seconds;
    uint64_t edges;
    uint32_t communities, levels;
} f2v_louvain_t;
typedef struct {
    double nmi, ari, mi, entropy_a, entropy_b, seconds;
    uint64_t n, sum_comb, sum_a, sum_b, total;
    uint32_t rows, cols;
} f2v_agreement_t;
F2V_API int f2v_louvain(f2v_handle h, uint64_t seed, uint32_t max_levels, uint32_t max_sweeps, uint32_t *labels_out /* n */,
                uint32_t *level_labels_out /* max_levels x n, may be NULL */, f2v_louvain_level_t *levels_out /* max_levels, may be NULL */,
                f2v_louvain_t *info_out);
F2V_API int f2v_partition_agreement(f2v_handle h, const uint32_t *a, uint32_t ka, const uint32_t *b, uint32_t kb, f2v_agreement_t *out);

/* ---- host-side I/O of the drop-in boundary (no device needed) ----------------------------
 * f2v_read_mtx replaces SetInputMatricesAsCSR (sample/commonutility.h:44-54 -> ReadASCII
 * sample/IO.h:59-156, CSC sample/CSC.h:146-188, CSR sample/CSR.h:154-186): MatrixMarket
 * coordinate text; "symmetric" mirrors off-diagonal entries and drops self-loops;
 * duplicates kept; colids ascending per row.  Arrays are malloc'ed; free with f2v_free. */
F2V_API int f2v_read_mtx(const char *path, uint32_t *n_out, uint64_t *nnz_out, uint32_t **rowptr_out, uint32_t **colids_out);
F2V_API void f2v_free(void *p);
/* Replaces algorithms::writeToFile (sample/algorithms.h:118-136): "<N> <D>\n", then
 * "<i+1> v0 v1 ... \n" with 6 significant digits (%g) and a trailing space. */
F2V_API int f2v_write_embd(const char *path, const float *x, uint32_t n, uint32_t dim);
/* Output file name rule of writeToFile + the per-option suffixes (sample/algorithms.cpp:650,
 * 752, 930, 1059, 1201, 1635, 2047, 2409, 2860): outdir + basename(input) + suffix + ".embd". */
F2V_API int f2v_output_name(const char *input, const char *outdir, int option, int bs_mode, uint32_t batch, uint32_t dim,
                    uint32_t iters, uint32_t ns, char *out, size_t out_len);

/* SURVEY 8f "next" rows on the data-format side of the path.
 * Binary CSR cache (text parsing of 10^8-edge files dominates wall time otherwise): little-endian
 * "F2VCSR1\0", u32 n, u32 reserved, u64 nnz, u32 rowptr[n+1], u32 colids[nnz] -- exactly the arrays
 * f2v_read_mtx returns, so a cached graph trains bit-identically. */
F2V_API int f2v_write_csr_bin(const char *path, const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint64_t nnz);
F2V_API int f2v_read_csr_bin(const char *path, uint32_t *n_out, uint64_t *nnz_out, uint32_t **rowptr_out, uint32_t **colids_out);
/* Raw fp32 N x D embedding file, the format the reference's scorers read with readBinEmbeddings
 * (performancescores/runnodeclassclust.py:81-100); text .embd of 16 M x 128 values is ~19 GB. */
F2V_API int f2v_write_embd_bin(const char *path, const float *x, uint32_t n, uint32_t dim);
/* The readers of both embedding formats (what performancescores/runnodeclassclust.py:57-100 reads): warm starts
 * (f2v_set_embeddings; `Force2Vec -init <file>`) and scoring without the text round trip.  f2v_read_embd allocates *x_out (N x D
 * floats, release with f2v_free); rows may come in any order, ids are 1-based. */
F2V_API int f2v_read_embd(const char *path, uint32_t *n_out, uint32_t *dim_out, float **x_out);
F2V_API int f2v_read_embd_bin(const char *path, uint32_t n, uint32_t dim, float *x_out);

/* Stand-alone libc rand() stream (glibc TYPE_3), for hosts that pre-draw sample ids. */
typedef struct f2v_rng f2v_rng;
F2V_API f2v_rng *f2v_rng_create(uint32_t seed);
F2V_API void f2v_rng_destroy(f2v_rng *g);
F2V_API int f2v_rng_next(f2v_rng *g);
/* Skip k draws in O(log k) (the generator is linear: a 31x31 matrix over Z/2^32 per jump). */
F2V_API void f2v_rng_jump(f2v_rng *g, uint64_t k);
/* `count` values as randInitF (kind 0) / randInit (kind 1) would store them, drawn from ONE serial stream but filled
 * in parallel from jump-ahead states; the stream ends where `count` serial draws would leave it. */
F2V_API int f2v_rng_fill(f2v_rng *g, float *out, uint64_t count, int kind);

/* One epoch's option-7 walk samples uint32[5*n] from stream g, exactly the reference's draws in the reference's order
 * (sample/algorithms.cpp:1097-1118) -- what f2v_generate_walks does with the handle's own stream, without a device. */
F2V_API int f2v_rng_walks(f2v_rng *g, const uint32_t *rowptr, const uint32_t *colids, uint32_t n, uint64_t nnz, uint32_t *walks_out);

/* The 2048-entry sigmoid table of init_SM_TABLE (sample/algorithms.cpp:757-764) as the source defines it. */
F2V_API int f2v_sm_table(float *table_out /* 2048 */);

/* ---- diagnostics (bench.py, tools/ipc_preflight.py, bin/Force2Vec -gpus) ------------------ */
/* Rehearsal of the push exchange's needs (IPC mapping of `bytes` of device memory and of fine-grained flags between
 * `world` processes that meet through files in `dir`, remote stores from a kernel), for a throw-away process to run
 * before the real engines exist: a mapping call that never returns or a faulting remote store then costs only it. */
F2V_API int f2v_diag_ipc_preflight(int device, uint32_t rank, uint32_t world, const char *dir, uint64_t bytes, double timeout_s);
/* On-box streaming-copy ceiling: read + written bytes per second (GB/s) of a 16-byte-per-lane copy of `bytes`, best of `reps`. */
F2V_API int f2v_diag_stream_copy(int device, uint64_t bytes, uint32_t reps, double *gbps_out);
/* On-box random-row gather ceiling (GB/s, ids included): every 512-byte row of a `table_bytes` table fetched once per pass
 * in random order with the step kernel's access pattern.  32 MiB: the Infinity Cache / L2 rate; 4 GiB: the HBM rate. */
F2V_API int f2v_diag_gather_rate(int device, uint64_t table_bytes, uint32_t reps, double *gbps_out);

#ifdef __cplusplus
}
#endif
#endif /* F2V_H_ */
