"""ctypes binding of libf2v.so (include/f2v.h).  The library is built in-tree by `make`
(or __graft_entry__.build()); there is no fallback implementation -- a missing library
is an ImportError, a missing GPU is F2V_ENODEV from f2v_create."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libf2v.so")
SELFTEST_LIB_PATH = os.path.join(HERE, "libf2v_selftest.so")

F2V_OK, F2V_EINVAL, F2V_ENODEV, F2V_ENOMEM, F2V_EIO, F2V_ESTATE = 0, -1, -2, -3, -4, -5
INIT_SYMMETRIC, INIT_UNIT = 0, 1
SIM_DOT, SIM_L2, SIM_COSINE = 0, 1, 2
NEAREST_MAX_K = 128
NEAREST_EXCLUDE_SELF, NEAREST_EXCLUDE_NEIGHBOURS = 1, 2
NEAREST_PAD_ID = 0xFFFFFFFF  # id of a slot past the last candidate (its score is -inf)
KMEANS_MAX_K, KMEANS_PIECE = 1024, 64
INDEX_MAX_LISTS, INDEX_MAX_PROBES = 1024, 128
LOGREG_MAX_CLASSES, LOGREG_BLOCK = 64, 1024
PAIR_HADAMARD, PAIR_L1, PAIR_L2, PAIR_AVERAGE = 0, 1, 2, 3
LABEL_NONE = 0xFFFFFFFF  # F2V_LABEL_NONE: the vertex takes no part in a separation score
SEPARATION_MAX_CLUSTERS, SEPARATION_PIECE, SEPARATION_SPAN = 1024, 64, 64
PCA_PIECE, TRUST_MAX_DIM = 4096, 512
FOLD_INIT_MEAN, FOLD_INIT_RANDOM, FOLD_INIT_GIVEN = 0, 1, 2
TSNE_PIECE, TSNE_SPAN = 64, 16
LOUVAIN_PHASES, AGREEMENT_MAX_CELLS, AGREEMENT_PIECE = 8, 1 << 26, 1024

u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
u8p = C.POINTER(C.c_uint8)


class Stats(C.Structure):
    _fields_ = [("step_launches", C.c_uint64), ("rows", C.c_uint64), ("nnz", C.c_uint64),
                ("algorithmic_bytes", C.c_uint64), ("device_seconds", C.c_double),
                ("hub_rows", C.c_uint64), ("hub_chunks", C.c_uint64), ("compulsory_bytes", C.c_uint64),
                ("snapshot_seconds", C.c_double), ("recoveries", C.c_uint64), ("recovered", C.c_uint32), ("merge_finalize", C.c_uint32)]


class Objective(C.Structure):  # f2v_objective_t
    _fields_ = [("loss", C.c_double), ("attraction", C.c_double), ("repulsion", C.c_double),
                ("positive_pairs", C.c_uint64), ("negative_pairs", C.c_uint64)]


class KMeansInfo(C.Structure):  # f2v_kmeans_t
    _fields_ = [("inertia", C.c_double), ("seconds", C.c_double), ("iterations", C.c_uint32), ("converged", C.c_uint32),
                ("restart", C.c_uint32), ("reserved", C.c_uint32)]


class IndexInfo(C.Structure):  # f2v_index_t
    _fields_ = [("inertia", C.c_double), ("seconds", C.c_double), ("bytes", C.c_uint64), ("lists", C.c_uint32), ("iterations", C.c_uint32),
                ("converged", C.c_uint32), ("largest", C.c_uint32), ("empty", C.c_uint32), ("reserved", C.c_uint32)]


class IndexSearchInfo(C.Structure):  # f2v_index_search_t
    _fields_ = [("seconds", C.c_double), ("candidates", C.c_uint64), ("nprobe", C.c_uint32), ("reserved", C.c_uint32)]


class LogregInfo(C.Structure):  # f2v_logreg_t
    _fields_ = [("loss", C.c_double), ("gnorm_inf", C.c_double), ("seconds", C.c_double), ("iterations", C.c_uint32),
                ("evaluations", C.c_uint32), ("converged", C.c_uint32), ("reserved", C.c_uint32)]


class PcaInfo(C.Structure):  # f2v_pca_t
    _fields_ = [("total_variance", C.c_double), ("seconds", C.c_double), ("sweeps", C.c_uint32), ("converged", C.c_uint32)]


class TrustInfo(C.Structure):  # f2v_trust_t
    _fields_ = [("trustworthiness", C.c_double), ("continuity", C.c_double), ("overlap", C.c_double), ("seconds", C.c_double),
                ("penalty_x", C.c_uint64), ("penalty_y", C.c_uint64), ("hits", C.c_uint64)]


class TsneParams(C.Structure):  # f2v_tsne_params
    _fields_ = [("perplexity", C.c_double), ("exaggeration", C.c_double), ("learning_rate", C.c_double), ("iters", C.c_uint32),
                ("exaggeration_iters", C.c_uint32), ("kl_every", C.c_uint32), ("reserved", C.c_uint32)]


class TsneInfo(C.Structure):  # f2v_tsne_t
    _fields_ = [("kl", C.c_double), ("z", C.c_double), ("learning_rate", C.c_double), ("seconds", C.c_double), ("nnz", C.c_uint64),
                ("k", C.c_uint32), ("reserved", C.c_uint32)]


class FoldInfo(C.Structure):  # f2v_fold_t
    _fields_ = [("seconds", C.c_double), ("pairs", C.c_uint64), ("resident", C.c_uint32), ("reserved", C.c_uint32)]


class LinkInfo(C.Structure):  # f2v_link_t
    _fields_ = [("seconds", C.c_double), ("positives", C.c_uint64), ("negatives", C.c_uint64), ("candidates", C.c_uint64), ("capped", C.c_uint64)]


class SplitInfo(C.Structure):  # f2v_split_t
    _fields_ = [("seconds", C.c_double), ("edges", C.c_uint64), ("candidates_held", C.c_uint64), ("protected_edges", C.c_uint64), ("held", C.c_uint64),
                ("train_nnz", C.c_uint64), ("negatives", C.c_uint64), ("drawn", C.c_uint64), ("capped", C.c_uint64)]


class RankingInfo(C.Structure):  # f2v_ranking_t
    _fields_ = [("auc", C.c_double), ("ap", C.c_double), ("concordant", C.c_uint64), ("tied", C.c_uint64), ("positives", C.c_uint64),
                ("negatives", C.c_uint64), ("groups", C.c_uint64), ("seconds", C.c_double)]


class PairRanksInfo(C.Structure):  # f2v_pair_ranks_t
    _fields_ = [("seconds", C.c_double), ("pairs", C.c_uint64), ("rank2_sum", C.c_uint64), ("mean_rank", C.c_double), ("mrr", C.c_double),
                ("candidates", C.c_uint64), ("tied_pairs", C.c_uint64)]


class ComponentsInfo(C.Structure):  # f2v_components_t
    _fields_ = [("seconds", C.c_double), ("edges", C.c_uint64), ("components", C.c_uint32), ("isolated", C.c_uint32), ("largest", C.c_uint32),
                ("largest_label", C.c_uint32), ("rounds", C.c_uint32)]


class ForestInfo(C.Structure):  # f2v_forest_t
    _fields_ = [("seconds", C.c_double), ("edges", C.c_uint64), ("forest_edges", C.c_uint64), ("components", C.c_uint32), ("rounds", C.c_uint32)]


class LouvainLevel(C.Structure):  # f2v_louvain_level_t
    _fields_ = [("nodes", C.c_uint32), ("communities", C.c_uint32), ("sweeps", C.c_uint32), ("reserved", C.c_uint32), ("moves", C.c_uint64),
                ("qnum", C.c_int64)]


class LouvainInfo(C.Structure):  # f2v_louvain_t
    _fields_ = [("modularity", C.c_double), ("seconds", C.c_double), ("edges", C.c_uint64), ("communities", C.c_uint32), ("levels", C.c_uint32)]


class AgreementInfo(C.Structure):  # f2v_agreement_t
    _fields_ = [("nmi", C.c_double), ("ari", C.c_double), ("mi", C.c_double), ("entropy_a", C.c_double), ("entropy_b", C.c_double),
                ("seconds", C.c_double), ("n", C.c_uint64), ("sum_comb", C.c_uint64), ("sum_a", C.c_uint64), ("sum_b", C.c_uint64),
                ("total", C.c_uint64), ("rows", C.c_uint32), ("cols", C.c_uint32)]


# every entry point declared in include/f2v.h: name -> (restype, argtypes)
SIGNATURES = {
    "f2v_last_error": (C.c_char_p, []),
    "f2v_version": (C.c_char_p, []),
    "f2v_create": (C.c_int, [u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "f2v_destroy": (C.c_int, [C.c_void_p]),
    "f2v_srand": (C.c_int, [C.c_void_p, C.c_uint32]),
    "f2v_init_embeddings": (C.c_int, [C.c_void_p, C.c_int]),
    "f2v_set_embeddings": (C.c_int, [C.c_void_p, f32p]),
    "f2v_get_embeddings": (C.c_int, [C.c_void_p, f32p]),
    "f2v_set_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "f2v_get_param": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "f2v_train": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.POINTER(C.c_double)]),
    "f2v_minibatch_step": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int]),
    "f2v_upload_sample_ids": (C.c_int, [C.c_void_p, u32p, C.c_uint64]),
    "f2v_minibatch_step_at": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float, C.c_int]),
    "f2v_flush": (C.c_int, [C.c_void_p]),
    "f2v_set_walks": (C.c_int, [C.c_void_p, u32p]),
    "f2v_generate_walks": (C.c_int, [C.c_void_p, u32p]),
    "f2v_rand_index": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, u32p]),
    "f2v_rand_indices": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u32p]),
    "f2v_stage_device_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), u32p]),
    "f2v_stage_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, f32p]),
    "f2v_stage_write": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, f32p]),
    "f2v_stage_reserve": (C.c_int, [C.c_void_p, C.c_uint32]),
    "f2v_rows_read": (C.c_int, [C.c_void_p, u32p, C.c_uint32, f32p]),
    "f2v_rows_write": (C.c_int, [C.c_void_p, u32p, C.c_uint32, f32p]),
    "f2v_embeddings_device_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "f2v_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "f2v_synchronize": (C.c_int, [C.c_void_p]),
    "f2v_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "f2v_train_marks": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, u32p]),
    "f2v_objective": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(Objective)]),
    "f2v_train_losses": (C.c_int, [C.c_void_p, u32p, C.POINTER(C.c_double), C.c_uint32, u32p]),
    "f2v_nearest_rows": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, u32p, f32p, C.POINTER(C.c_double)]),
    "f2v_nearest_vectors": (C.c_int, [C.c_void_p, f32p, C.c_uint32, C.c_uint32, C.c_int, u32p, f32p, C.POINTER(C.c_double)]),
    "f2v_neighbour_recall": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "f2v_kmeans": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, f32p, u32p, f32p, C.POINTER(C.c_uint64), C.POINTER(KMeansInfo)]),
    "f2v_modularity": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "f2v_index_build": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, f32p, C.POINTER(IndexInfo)]),
    "f2v_index_build_given": (C.c_int, [C.c_void_p, u32p, f32p, C.c_uint32, C.POINTER(IndexInfo)]),
    "f2v_index_get": (C.c_int, [C.c_void_p, u32p, f32p, C.POINTER(C.c_uint64), C.POINTER(IndexInfo)]),
    "f2v_index_drop": (C.c_int, [C.c_void_p]),
    "f2v_index_search_rows": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u32p, f32p, u32p, C.POINTER(IndexSearchInfo)]),
    "f2v_index_search_vectors": (C.c_int, [C.c_void_p, f32p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, u32p, f32p, u32p, C.POINTER(IndexSearchInfo)]),
    "f2v_logreg_eval": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32, C.c_int, u8p, C.c_uint32, f64p, C.c_double, f64p, f64p, f64p]),
    "f2v_logreg_fit": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32, C.c_int, u8p, C.c_uint32, C.c_double, C.c_double, C.c_uint32, f64p, C.POINTER(LogregInfo)]),
    "f2v_logreg_decision": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32, C.c_int, f64p, C.c_uint32, f64p, f64p]),
    "f2v_silhouette": (C.c_int, [C.c_void_p, u32p, C.c_uint32, u32p, C.c_uint32, f64p, u32p, f64p, f64p]),
    "f2v_davies_bouldin": (C.c_int, [C.c_void_p, u32p, C.c_uint32, f64p, f32p, f64p, C.POINTER(C.c_uint64), f64p]),
    "f2v_pca": (C.c_int, [C.c_void_p, C.c_uint32, f32p, f64p, f64p, f64p, C.POINTER(PcaInfo)]),
    "f2v_trustworthiness": (C.c_int, [C.c_void_p, f32p, C.c_uint32, C.c_uint32, u32p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(TrustInfo)]),
    "f2v_tsne_affinities": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.c_double, u32p, u32p, f64p, C.c_uint64, C.POINTER(C.c_uint64), f64p]),
    "f2v_tsne": (C.c_int, [C.c_void_p, u32p, C.c_uint32, C.c_uint32, C.POINTER(TsneParams), u32p, u32p, f64p, f64p, f32p, C.POINTER(TsneInfo)]),
    "f2v_tsne_kl_log": (C.c_int, [C.c_void_p, u32p, f64p, C.c_uint32, u32p]),
    "f2v_fold_in": (C.c_int, [C.c_void_p, C.c_int, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, f32p, C.c_uint64, C.c_uint64, f32p, C.POINTER(FoldInfo)]),
    "f2v_link_pairs": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, u32p, u32p, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(LinkInfo)]),
    "f2v_edge_split": (C.c_int, [C.c_void_p, C.c_double, C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint64, u32p, u32p, C.c_uint64, u32p, u32p, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(SplitInfo)]),
    "f2v_edge_split_connected": (C.c_int, [C.c_void_p, C.c_double, C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint64, u32p, u32p, C.c_uint64, u32p, u32p, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(SplitInfo)]),
    "f2v_components": (C.c_int, [C.c_void_p, u32p, u32p, C.POINTER(ComponentsInfo)]),
    "f2v_spanning_forest": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(ForestInfo)]),
    "f2v_forest_round_seconds": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, u32p]),
    "f2v_subgraph": (C.c_int, [C.c_void_p, u8p, u32p, u32p, C.c_uint64, u32p, u32p, C.POINTER(C.c_uint64)]),
    "f2v_pair_scores": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint64, C.c_int, f32p, C.POINTER(C.c_double)]),
    "f2v_ranking": (C.c_int, [C.c_void_p, f64p, u8p, C.c_uint64, C.POINTER(RankingInfo)]),
    "f2v_pair_neighbourhood": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint64, C.c_uint32, f64p, C.POINTER(C.c_double)]),
    "f2v_pair_ranks": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint64, C.c_int, C.c_uint32, u32p, u32p, u32p, C.c_uint32, C.POINTER(C.c_uint64),
                                 C.POINTER(PairRanksInfo)]),
    "f2v_louvain": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u32p, C.POINTER(LouvainLevel), C.POINTER(LouvainInfo)]),
    "f2v_partition_agreement": (C.c_int, [C.c_void_p, u32p, C.c_uint32, u32p, C.c_uint32, C.POINTER(AgreementInfo)]),
    "f2v_push_export": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f2v_push_attach": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "f2v_push_selftest": (C.c_int, [C.c_void_p]),
    "f2v_push_detach": (C.c_int, [C.c_void_p]),
    "f2v_train_sharded": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.POINTER(C.c_double)]),
    "f2v_shard_bounds": (C.c_int, [u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
    "f2v_push_masks": (C.c_int, [u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint64, u32p]),
    "f2v_push_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "f2v_read_mtx": (C.c_int, [C.c_char_p, u32p, C.POINTER(C.c_uint64), C.POINTER(u32p), C.POINTER(u32p)]),
    "f2v_free": (None, [C.c_void_p]),
    "f2v_write_embd": (C.c_int, [C.c_char_p, f32p, C.c_uint32, C.c_uint32]),
    "f2v_write_csr_bin": (C.c_int, [C.c_char_p, u32p, u32p, C.c_uint32, C.c_uint64]),
    "f2v_read_csr_bin": (C.c_int, [C.c_char_p, u32p, C.POINTER(C.c_uint64), C.POINTER(u32p), C.POINTER(u32p)]),
    "f2v_write_embd_bin": (C.c_int, [C.c_char_p, f32p, C.c_uint32, C.c_uint32]),
    "f2v_read_embd": (C.c_int, [C.c_char_p, u32p, u32p, C.POINTER(f32p)]),
    "f2v_read_embd_bin": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, f32p]),
    "f2v_output_name": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "f2v_rng_create": (C.c_void_p, [C.c_uint32]),
    "f2v_rng_destroy": (None, [C.c_void_p]),
    "f2v_rng_next": (C.c_int, [C.c_void_p]),
    "f2v_rng_jump": (None, [C.c_void_p, C.c_uint64]),
    "f2v_rng_fill": (C.c_int, [C.c_void_p, f32p, C.c_uint64, C.c_int]),
    "f2v_rng_walks": (C.c_int, [C.c_void_p, u32p, u32p, C.c_uint32, C.c_uint64, u32p]),
    "f2v_sm_table": (C.c_int, [f32p]),
    "f2v_diag_ipc_preflight": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_double]),
    "f2v_diag_stream_copy": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "f2v_diag_gather_rate": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
}

# include/f2v_test.h: only in libf2v_selftest.so (the same sources built with -DF2V_TEST_HOOKS), for tests/ and tools/
TEST_SIGNATURES = {
    "f2v_test_push_attach_local": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "f2v_test_gather_calibration": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32]),
    "f2v_test_wave_reduce": (C.c_int, [C.c_int, f32p, C.c_uint32, C.c_uint32, f32p]),
    "f2v_test_withhold_flag": (C.c_int, [C.c_void_p, C.c_uint32]),
    "f2v_test_chain_nowait": (C.c_int, [C.c_void_p, C.c_int]),
    "f2v_test_withhold_row": (C.c_int, [C.c_void_p, C.c_uint32]),
    "f2v_test_stamps": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "f2v_test_xcd_times": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "f2v_test_plan_gather": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "f2v_test_interaction_stub": (C.c_int, [C.c_void_p, C.c_uint32]),
    "f2v_test_pca_scatter": (C.c_int, [C.c_void_p, f64p, f64p]),
    "f2v_test_wide_plan_check": (C.c_int, [u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_uint32, C.POINTER(C.c_uint64)]),
}

PUSH_EXPORT_BYTES = 256  # F2V_PUSH_EXPORT_BYTES
PUSH_MAX_RANKS = 8       # F2V_PUSH_MAX_RANKS

_lib = None
_selftest = None


class F2VError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libf2v error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("F2V_LIBRARY", LIB_PATH)  # A/B runs of two builds of the library
        if not os.path.exists(path):
            raise ImportError("%s is missing: build it with `make` (hipcc --offload-arch=gfx950); "
                              "force2vec_amd has no fallback implementation" % path)
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            if path != LIB_PATH and not hasattr(L, name):
                continue  # an older build in an A/B run
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def selftest_lib():
    """The self-test build (fault injection, look-inside hooks): a library of its own, with its own handles."""
    global _selftest
    if _selftest is None:
        path = os.environ.get("F2V_SELFTEST_LIBRARY", SELFTEST_LIB_PATH)  # A/B runs of two self-test builds
        if not os.path.exists(path):
            raise ImportError("%s is missing: build it with `make`" % path)
        L = C.CDLL(path)
        for table in (SIGNATURES, TEST_SIGNATURES):
            for name, (res, args) in table.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        _selftest = L
    return _selftest


def check(rc, L=None):
    if rc != F2V_OK:
        raise F2VError(rc, (L or lib()).f2v_last_error().decode(errors="replace"))
