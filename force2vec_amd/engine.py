"""Host-side mirror of the reference's operator interface over libf2v (include/f2v.h).

`Engine` is the thin handle wrapper; `algorithms` mirrors `class algorithms` of
sample/algorithms.h:51-137 -- same constructor meaning, same AlgoForce2Vec* method names and
(ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr) arguments, result [seconds], side effect = the
.embd file -- so the parity tests read like a user of the reference.  All force arithmetic
runs in the HIP kernels; nothing here (or anywhere in this package) computes on the CPU."""
import ctypes as C
import os
import time
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import INIT_SYMMETRIC, INIT_UNIT, check


# f2v_objective_t (include/f2v.h): loss = attraction + repulsion; the pair counts are the kernel's work proof (nnz, n * ns)
Objective = namedtuple("Objective", "loss attraction repulsion positive_pairs negative_pairs")


# Engine.kmeans / Engine.modularity (include/f2v.h: clustering)
KMeans = namedtuple("KMeans", "labels centroids inertia iterations converged restart counts")
Modularity = namedtuple("Modularity", "q edges inside degree")
IndexInfo = namedtuple("IndexInfo", "lists inertia iterations converged largest empty bytes seconds")


# Engine.pca / Engine.trustworthiness (include/f2v.h: layout)
Pca = namedtuple("Pca", "y components mean variance info")
PcaInfo = namedtuple("PcaInfo", "total_variance seconds sweeps converged")
Trust = namedtuple("Trust", "trustworthiness continuity overlap penalty_x penalty_y hits seconds samples_x samples_y")


# Engine.fold_in (include/f2v.h: fold-in)
FoldInfo = namedtuple("FoldInfo", "seconds pairs resident")
FOLD_INITS = {"mean": _lib.FOLD_INIT_MEAN, "random": _lib.FOLD_INIT_RANDOM}


# Engine.link_pairs (include/f2v.h: link prediction pairs)
LinkInfo = namedtuple("LinkInfo", "seconds positives negatives candidates capped")
EdgeSplit = namedtuple("EdgeSplit", "rowptr colids held_u held_v neg_u neg_v")
EdgeSplitDetails = namedtuple("EdgeSplitDetails", "rowptr colids held_u held_v neg_u neg_v info")
SplitInfo = namedtuple("SplitInfo", "seconds edges candidates_held protected held train_nnz negatives drawn capped")
Components = namedtuple("Components", "sizes components isolated largest largest_label edges rounds seconds")
Forest = namedtuple("Forest", "seconds edges forest_edges components rounds round_seconds")
Subgraph = namedtuple("Subgraph", "rowptr colids ids new_id")
Ranking = namedtuple("Ranking", "auc ap concordant tied positives negatives groups seconds")
HeldoutScores = namedtuple("HeldoutScores", "auc ap classifier_auc classifier_ap")
PairRanks = namedtuple("PairRanks", "greater equal mrr mean_rank hits candidates tied_pairs seconds")
# Engine.communities, Engine.agreement (include/f2v.h: communities)
Communities = namedtuple("Communities", "modularity communities levels edges seconds level_records level_labels")
LouvainLevel = namedtuple("LouvainLevel", "nodes communities sweeps moves qnum")
Agreement = namedtuple("Agreement", "nmi ari mi entropy_a entropy_b n sum_comb sum_a sum_b total rows cols seconds")


# Engine.logreg_fit / Engine.classify / Engine.link_predict (include/f2v.h: logistic regression)
LogregModel = namedtuple("LogregModel", "weights feature loss gnorm_inf iterations evaluations converged seconds")
F1 = namedtuple("F1", "micro macro")
LinkScores = namedtuple("LinkScores", "accuracy f1_macro f1_micro")
PAIR_FEATURES = {"hadamard": _lib.PAIR_HADAMARD, "l1": _lib.PAIR_L1, "l2": _lib.PAIR_L2, "average": _lib.PAIR_AVERAGE}


def _f1(true, pred, classes):
    """micro / macro F1 in percent of 0/1 matrices [samples, len(classes)] over the given class columns (a class without a
    prediction and without a true label scores 0, as scikit-learn's f1_score does)."""
    t, p = true[:, classes].astype(bool), pred[:, classes].astype(bool)
    tp, fp, fn = (t & p).sum(0).astype(np.float64), (~t & p).sum(0).astype(np.float64), (t & ~p).sum(0).astype(np.float64)
    den = 2 * tp + fp + fn
    per = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    den_all = 2 * tp.sum() + fp.sum() + fn.sum()
    return F1(100.0 * (2 * tp.sum() / den_all if den_all > 0 else 0.0), 100.0 * (sum(per.tolist()) / len(classes)) if len(classes) else 0.0)


METRICS = {"dot": _lib.SIM_DOT, "l2": _lib.SIM_L2, "cos": _lib.SIM_COSINE, "cosine": _lib.SIM_COSINE}
# the kinds of f2v_pair_neighbourhood (F2V_NB_*), in the order of their bits: the order of the result arrays
NEIGHBOURHOOD_KINDS = {"cn": 1, "jaccard": 2, "aa": 4, "ra": 8, "pa": 16}


def _u32(a):
    return a.ctypes.data_as(_lib.u32p)


def _f32(a):
    return a.ctypes.data_as(_lib.f32p)


class Engine:
    """One HBM-resident graph + embedding matrix on one MI355X."""

    def __init__(self, rowptr, colids, dim, device=0, selftest=False):
        # selftest: bind this engine to libf2v_selftest.so (include/f2v_test.h), e.g. for fault injection
        self._L = _lib.selftest_lib() if selftest else _lib.lib()
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint32)
        colids = np.ascontiguousarray(colids, dtype=np.uint32)
        self.n = len(rowptr) - 1
        self.nnz = int(rowptr[-1])
        self.dim = int(dim)
        self.rowptr, self.colids = rowptr, colids
        h = C.c_void_p()
        self._ck(self._L.f2v_create(_u32(rowptr), _u32(colids), self.n, self.nnz, self.dim, device, C.byref(h)))
        self._h = h
        self.last_nearest_seconds = self.last_kmeans_seconds = self.last_logreg_seconds = 0.0  # device time of the last query / clustering / regression call
        self.last_separation_seconds = 0.0  # ... / silhouette or Davies-Bouldin call
        self.last_layout_seconds = 0.0  # ... / pca or trustworthiness call
        self.last_fold_seconds = 0.0  # ... / fold_in call
        self.last_link_seconds = 0.0  # ... / link_pairs call (its count and its fill together)
        self.last_louvain_seconds = 0.0  # ... / communities call
        self.last_components_seconds = self.last_forest_seconds = self.last_subgraph_seconds = 0.0  # ... / components, spanning_forest, subgraph call

    def _ck(self, rc):
        check(rc, self._L)  # the error text lives in the library that returned the code

    def close(self):
        if getattr(self, "_h", None):
            self._L.f2v_destroy(self._h)
            self._h = None

    __del__ = close

    # -- rand() stream / embeddings ---------------------------------------------------------
    def srand(self, seed=1):
        self._ck(self._L.f2v_srand(self._h, seed))

    def init_embeddings(self, kind):
        self._ck(self._L.f2v_init_embeddings(self._h, kind))

    def set_embeddings(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        assert X.shape == (self.n, self.dim)
        self._ck(self._L.f2v_set_embeddings(self._h, _f32(X)))

    def get_embeddings(self):
        X = np.empty((self.n, self.dim), dtype=np.float32)
        self._ck(self._L.f2v_get_embeddings(self._h, _f32(X)))
        return X

    def rand_index(self, max_num, min_num=0):
        out = C.c_uint32()
        self._ck(self._L.f2v_rand_index(self._h, max_num, min_num, C.byref(out)))
        return out.value

    def draw_samples(self, max_num, count, keep=None):
        """`count` randIndex(max_num, 0) draws from the handle's rand() stream; the first `keep` are returned."""
        keep = count if keep is None else keep
        out = np.empty(max(keep, 1), dtype=np.uint32)
        self._ck(self._L.f2v_rand_indices(self._h, max_num, 0, count, keep, _u32(out)))
        return out[:keep]

    def set_param(self, name, value):
        self._ck(self._L.f2v_set_param(self._h, name.encode(), int(value)))

    def get_param(self, name):
        v = C.c_int64()
        self._ck(self._L.f2v_get_param(self._h, name.encode(), C.byref(v)))
        return v.value

    # -- training -----------------------------------------------------------------------------
    def train(self, option, iters, batch, ns=5, lr=0.02, bs_mode=0):
        """-> device seconds of the epoch loop."""
        sec = C.c_double()
        self._ck(self._L.f2v_train(self._h, option, iters, batch, ns, lr, bs_mode, C.byref(sec)))
        return sec.value

    # -- multi-GPU push exchange over xGMI (include/f2v.h) ----------------------------------------
    def push_export(self):
        """-> bytes: this rank's IPC handles (gather them from all ranks, then push_attach)."""
        buf = C.create_string_buffer(_lib.PUSH_EXPORT_BYTES)
        self._ck(self._L.f2v_push_export(self._h, buf))
        return buf.raw

    def push_attach(self, rank, world, exports):
        blob = b"".join(exports)
        assert len(blob) == world * _lib.PUSH_EXPORT_BYTES
        self._ck(self._L.f2v_push_attach(self._h, rank, world, C.c_char_p(blob)))

    def push_selftest(self):
        self._ck(self._L.f2v_push_selftest(self._h))

    def push_detach(self):
        self._ck(self._L.f2v_push_detach(self._h))

    def push_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.f2v_push_stats(self._h, C.byref(a), C.byref(b)))
        return {"rows_pushed": a.value, "rows_allgather": b.value}

    def train_sharded(self, option, iters, batch, ns=5, lr=0.02, bs_mode=0):
        """f2v_train over the attached ranks -> device seconds of the epoch loop (exchange included)."""
        sec = C.c_double()
        self._ck(self._L.f2v_train_sharded(self._h, option, iters, batch, ns, lr, bs_mode, C.byref(sec)))
        return sec.value

    def minibatch_step(self, option, batch_lo, batch_hi, sample_ids, ns, lr, bs_mode=0, row_lo=None, row_hi=None):
        ids = np.ascontiguousarray(sample_ids, dtype=np.uint32)
        self._ck(self._L.f2v_minibatch_step(self._h, option, batch_lo, batch_hi,
                                         batch_lo if row_lo is None else row_lo, batch_hi if row_hi is None else row_hi,
                                         _u32(ids), len(ids), ns, lr, bs_mode))

    def upload_sample_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self._ck(self._L.f2v_upload_sample_ids(self._h, _u32(ids), len(ids)))

    def minibatch_step_at(self, option, batch_lo, batch_hi, ids_offset, ns, lr, bs_mode=0, row_lo=None, row_hi=None):
        self._ck(self._L.f2v_minibatch_step_at(self._h, option, batch_lo, batch_hi,
                                            batch_lo if row_lo is None else row_lo, batch_hi if row_hi is None else row_hi,
                                            ids_offset, ns, lr, bs_mode))

    def flush(self):
        self._ck(self._L.f2v_flush(self._h))

    def synchronize(self):
        self._ck(self._L.f2v_synchronize(self._h))

    def set_walks(self, walks):
        w = np.ascontiguousarray(walks, dtype=np.uint32)
        assert w.size == 5 * self.n
        self._ck(self._L.f2v_set_walks(self._h, _u32(w)))

    def generate_walks(self):
        w = np.empty(5 * self.n, dtype=np.uint32)
        self._ck(self._L.f2v_generate_walks(self._h, _u32(w)))
        return w

    def stage_reserve(self, rows):
        self._ck(self._L.f2v_stage_reserve(self._h, rows))

    def stage_read(self, row_lo, row_hi):
        out = np.empty((row_hi - row_lo, self.dim), dtype=np.float32)
        self._ck(self._L.f2v_stage_read(self._h, row_lo, row_hi, _f32(out)))
        return out

    def stage_write(self, row_lo, row_hi, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.shape == (row_hi - row_lo, self.dim)
        self._ck(self._L.f2v_stage_write(self._h, row_lo, row_hi, _f32(rows)))

    def rows_read(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty((len(ids), self.dim), dtype=np.float32)
        self._ck(self._L.f2v_rows_read(self._h, _u32(ids), len(ids), _f32(out)))
        return out

    def rows_write(self, ids, rows):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.shape == (len(ids), self.dim)
        self._ck(self._L.f2v_rows_write(self._h, _u32(ids), len(ids), _f32(rows)))

    def embeddings_device_ptr(self):
        p = C.c_uint64()
        self._ck(self._L.f2v_embeddings_device_ptr(self._h, C.byref(p)))
        return p.value

    def stage_device_ptr(self):
        p = C.c_uint64()
        cap = C.c_uint32()
        self._ck(self._L.f2v_stage_device_ptr(self._h, C.byref(p), C.byref(cap)))
        return p.value, cap.value

    def stream(self):
        s = C.c_uint64()
        self._ck(self._L.f2v_stream(self._h, C.byref(s)))
        return s.value

    def train_marks(self):
        """Device seconds from the start of the last f2v_train's epoch loop to every "epoch_marks"-th epoch's end."""
        n = C.c_uint32()
        self._ck(self._L.f2v_train_marks(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.float64)
        self._ck(self._L.f2v_train_marks(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return out[: n.value]

    def objective(self, option, ns=5):
        """The training objective of the current matrix (include/f2v.h: definition; deterministic) -> Objective."""
        o = _lib.Objective()
        self._ck(self._L.f2v_objective(self._h, option, ns, C.byref(o)))
        return Objective(o.loss, o.attraction, o.repulsion, o.positive_pairs, o.negative_pairs)

    def train_losses(self):
        """The last f2v_train's "loss_every" log -> (epochs uint32[k], 1-based; values float64[k, 3]: loss, attraction, repulsion)."""
        n = C.c_uint32()
        self._ck(self._L.f2v_train_losses(self._h, None, None, 0, C.byref(n)))
        epochs = np.zeros(max(n.value, 1), dtype=np.uint32)
        values = np.zeros((max(n.value, 1), 3), dtype=np.float64)
        self._ck(self._L.f2v_train_losses(self._h, _u32(epochs), values.ctypes.data_as(C.POINTER(C.c_double)), n.value, C.byref(n)))
        return epochs[: n.value], values[: n.value]

    # -- nearest neighbours (include/f2v.h: definition; a function of the matrix, the metric, k and the flags alone) --------------
    def nearest(self, ids=None, vectors=None, k=10, metric="dot", exclude_self=True, exclude_neighbours=False):
        """The k most similar rows of the matrix for each query -> (ids uint32 [nq, k], scores float32 [nq, k]).  Queries are
        the rows `ids` (default: all vertices) or the float32 `vectors` [nq, dim]; the two exclusions apply to rows only.
        metric: "dot" | "l2" | "cos".  Slots past the last candidate hold id 0xFFFFFFFF and score -inf.  `last_nearest_seconds`
        keeps the device time."""
        m = METRICS[metric] if isinstance(metric, str) else int(metric)
        sec = C.c_double()
        if vectors is not None:
            if ids is not None:
                raise ValueError("nearest: give ids or vectors, not both")
            q = np.ascontiguousarray(vectors, dtype=np.float32)
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise ValueError("nearest: vectors must be [nq, %d]" % self.dim)
            nq = q.shape[0]
            out_ids, out_scores = np.empty((nq, k), dtype=np.uint32), np.empty((nq, k), dtype=np.float32)
            self._ck(self._L.f2v_nearest_vectors(self._h, _f32(q), nq, k, m, _u32(out_ids), _f32(out_scores), C.byref(sec)))
        else:
            q = np.arange(self.n, dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            flags = (_lib.NEAREST_EXCLUDE_SELF if exclude_self else 0) | (_lib.NEAREST_EXCLUDE_NEIGHBOURS if exclude_neighbours else 0)
            out_ids, out_scores = np.empty((len(q), k), dtype=np.uint32), np.empty((len(q), k), dtype=np.float32)
            self._ck(self._L.f2v_nearest_rows(self._h, _u32(q), len(q), k, m, flags, _u32(out_ids), _f32(out_scores), C.byref(sec)))
        self.last_nearest_seconds = sec.value
        return out_ids, out_scores

    def neighbour_recall(self, k=10, metric="dot", ids=None):
        """Graph-reconstruction precision@k, counted on the device -> (hits, possible): how many of the vertices' top-k (self
        excluded) are their CSR neighbours, out of sum min(k, distinct neighbours).  ids=None: all vertices."""
        m = METRICS[metric] if isinstance(metric, str) else int(metric)
        hits, possible, sec = C.c_uint64(), C.c_uint64(), C.c_double()
        if ids is None:
            self._ck(self._L.f2v_neighbour_recall(self._h, None, 0, k, m, C.byref(hits), C.byref(possible), C.byref(sec)))
        else:
            q = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            self._ck(self._L.f2v_neighbour_recall(self._h, _u32(q), len(q), k, m, C.byref(hits), C.byref(possible), C.byref(sec)))
        self.last_nearest_seconds = sec.value
        return hits.value, possible.value

    # -- nearest neighbours through an index (include/f2v.h: definition; exact top-k over the members of the probed lists) ---------
    def build_index(self, lists=None, max_iters=20, seed=1, init=None, labels=None, centroids=None):
        """Partition the rows into `lists` lists for index_search -> IndexInfo.  By k-means on the matrix as it stands (the very
        labels and centroids kmeans(lists, max_iters, seed) returns; `init`: its initial centroids), or from the given `labels`
        (uint32 [n]) and `centroids` (float32 [lists, dim]).  lists=None: min(1024, max(1, round(sqrt(n)))), or the centroids'
        count in the given form.  The index keeps no copy of the matrix and is never rebuilt by itself."""
        info = _lib.IndexInfo()
        if (labels is None) != (centroids is None):
            raise ValueError("build_index: give labels and centroids together")
        if labels is not None:
            cen = np.ascontiguousarray(centroids, dtype=np.float32)
            lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
            if cen.ndim != 2 or cen.shape[1] != self.dim or len(lab) != self.n or (lists is not None and lists != cen.shape[0]):
                raise ValueError("build_index: labels must be [%d] and centroids [lists, %d]" % (self.n, self.dim))
            self._ck(self._L.f2v_index_build_given(self._h, _u32(lab), _f32(cen), cen.shape[0], C.byref(info)))
        else:
            if lists is None:
                lists = min(_lib.INDEX_MAX_LISTS, max(1, int(round(self.n ** 0.5))))
            c0 = None
            if init is not None:
                c0 = np.ascontiguousarray(init, dtype=np.float32)
                if c0.shape != (lists, self.dim):
                    raise ValueError("build_index: init must be [%d, %d]" % (lists, self.dim))
            self._ck(self._L.f2v_index_build(self._h, lists, max_iters, seed, _f32(c0) if c0 is not None else None, C.byref(info)))
        return IndexInfo(info.lists, info.inertia, info.iterations, bool(info.converged), info.largest, info.empty, info.bytes, info.seconds)

    def index(self):
        """The index as it stands -> (labels uint32 [n], centroids float32 [lists, dim], counts uint64 [lists])."""
        info = _lib.IndexInfo()
        self._ck(self._L.f2v_index_get(self._h, None, None, None, C.byref(info)))
        labels = np.empty(self.n, dtype=np.uint32)
        centroids = np.empty((info.lists, self.dim), dtype=np.float32)
        counts = np.empty(info.lists, dtype=np.uint64)
        self._ck(self._L.f2v_index_get(self._h, _u32(labels), _f32(centroids), counts.ctypes.data_as(C.POINTER(C.c_uint64)), None))
        return labels, centroids, counts

    def drop_index(self):
        self._ck(self._L.f2v_index_drop(self._h))

    def index_search(self, ids=None, vectors=None, k=10, metric="dot", nprobe=8, exclude_self=True, exclude_neighbours=False, details=False):
        """nearest() over the members of the `nprobe` lists whose centroids are nearest to each query -> (ids, scores), with
        `details` also (probes uint32 [nq, P], {"seconds", "candidates", "nprobe"}).  Same queries, metrics, exclusions, order and
        padding as nearest(); with nprobe >= lists the two are equal bit for bit.  `last_nearest_seconds` keeps the device time."""
        m = METRICS[metric] if isinstance(metric, str) else int(metric)
        ginfo, info = _lib.IndexInfo(), _lib.IndexSearchInfo()
        self._ck(self._L.f2v_index_get(self._h, None, None, None, C.byref(ginfo)))
        P = max(1, min(int(nprobe), ginfo.lists))
        if vectors is not None:
            if ids is not None:
                raise ValueError("index_search: give ids or vectors, not both")
            q = np.ascontiguousarray(vectors, dtype=np.float32)
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise ValueError("index_search: vectors must be [nq, %d]" % self.dim)
            nq = q.shape[0]
            out_ids, out_scores, probes = np.empty((nq, k), dtype=np.uint32), np.empty((nq, k), dtype=np.float32), np.empty((nq, P), dtype=np.uint32)
            self._ck(self._L.f2v_index_search_vectors(self._h, _f32(q), nq, k, m, nprobe, _u32(out_ids), _f32(out_scores), _u32(probes), C.byref(info)))
        else:
            q = np.arange(self.n, dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
            flags = (_lib.NEAREST_EXCLUDE_SELF if exclude_self else 0) | (_lib.NEAREST_EXCLUDE_NEIGHBOURS if exclude_neighbours else 0)
            out_ids, out_scores, probes = np.empty((len(q), k), dtype=np.uint32), np.empty((len(q), k), dtype=np.float32), np.empty((len(q), P), dtype=np.uint32)
            self._ck(self._L.f2v_index_search_rows(self._h, _u32(q), len(q), k, m, flags, nprobe, _u32(out_ids), _f32(out_scores), _u32(probes), C.byref(info)))
        self.last_nearest_seconds = info.seconds
        if details:
            return out_ids, out_scores, probes, {"seconds": info.seconds, "candidates": info.candidates, "nprobe": info.nprobe}
        return out_ids, out_scores

    def index_recall(self, k=10, metric="dot", nprobe=8, ids=None):
        """How many of nearest()'s top-k ids index_search finds for the vertices `ids` (default: all) -> (found, possible)."""
        want, _ = self.nearest(ids=ids, k=k, metric=metric)
        got, _ = self.index_search(ids=ids, k=k, metric=metric, nprobe=nprobe)
        found = 0
        for lo in range(0, len(want), 65536):  # set intersection per query (a row's ids are distinct), in blocks that bound the comparison table
            g, w = got[lo:lo + 65536], want[lo:lo + 65536]
            found += int(((g[:, None, :] == w[:, :, None]).any(axis=2) & (w != _lib.NEAREST_PAD_ID)).sum())
        return found, int((want != _lib.NEAREST_PAD_ID).sum())

    # -- clustering (include/f2v.h: definition; a function of the matrix, k, max_iters, restarts and the seed alone) -------------
    def kmeans(self, k, max_iters=300, seed=1, restarts=1, init=None):
        """Lloyd's k-means on the rows of the matrix, on the GPU -> KMeans(labels uint32[n], centroids float32[k, dim], inertia,
        iterations, converged, restart, counts uint64[k]).  Initial centroids: `init` (float32 [k, dim]) or rows drawn from `seed`;
        of `restarts` seeded runs (seed, seed + 1, ...) the one of lowest inertia is returned.  `last_kmeans_seconds` keeps the
        device time."""
        labels = np.empty(self.n, dtype=np.uint32)
        centroids = np.empty((k, self.dim), dtype=np.float32)
        counts = np.empty(k, dtype=np.uint64)
        c0 = None
        if init is not None:
            c0 = np.ascontiguousarray(init, dtype=np.float32)
            if c0.shape != (k, self.dim):
                raise ValueError("kmeans: init must be [%d, %d]" % (k, self.dim))
        info = _lib.KMeansInfo()
        self._ck(self._L.f2v_kmeans(self._h, k, max_iters, restarts, seed, _f32(c0) if c0 is not None else None, _u32(labels), _f32(centroids),
                                    counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info)))
        self.last_kmeans_seconds = info.seconds
        return KMeans(labels, centroids, info.inertia, info.iterations, bool(info.converged), info.restart, counts)

    def modularity(self, labels, n_clusters=None):
        """Newman modularity of `labels` on the simple undirected graph of the CSR, tallied on the GPU -> Modularity(q, edges,
        inside uint64[n_clusters], degree uint64[n_clusters]).  n_clusters=None: max(labels) + 1."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        if len(lab) != self.n:
            raise ValueError("modularity: one label per vertex")
        nc = (int(lab.max()) + 1 if len(lab) else 1) if n_clusters is None else int(n_clusters)
        q, edges = C.c_double(), C.c_uint64()
        inside, degree = np.zeros(max(nc, 1), dtype=np.uint64), np.zeros(max(nc, 1), dtype=np.uint64)
        self._ck(self._L.f2v_modularity(self._h, _u32(lab), nc, C.byref(q), C.byref(edges), inside.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        degree.ctypes.data_as(C.POINTER(C.c_uint64))))
        return Modularity(q.value, edges.value, inside[:nc], degree[:nc])

    # -- separation (include/f2v.h: definition; a function of the matrix, the labelling and the samples alone) ---------------------
    def _labelling(self, labels):
        """-> (uint32 labels with F2V_LABEL_NONE for negative entries, n_clusters = the largest label + 1)"""
        lab = np.asarray(labels).reshape(-1)
        if len(lab) != self.n or lab.dtype.kind not in "iu":
            raise ValueError("separation: one integer label per vertex")
        wide = lab.astype(np.int64)
        none = wide < 0 if lab.dtype.kind == "i" else lab == _lib.LABEL_NONE
        if lab.dtype.kind == "u":
            wide = np.where(none, -1, wide)
        out = np.where(none, _lib.LABEL_NONE, wide).astype(np.uint32)
        return np.ascontiguousarray(out), int(wide.max()) + 1 if len(wide) and wide.max() >= 0 else 1

    def silhouette(self, labels, ids=None, samples=False):
        """The silhouette of `labels` (any integer array, one per vertex; negative = the vertex takes no part) in the embedding
        space, on the GPU -> the mean s(i) over the samples `ids` (None: every labelled vertex), or with samples=True
        (score, s float64[len(ids)], other uint32[len(ids)]: the nearest other cluster of every sample).  Every sample is scored
        against all labelled vertices.  `last_separation_seconds` keeps the device time."""
        lab, nc = self._labelling(labels)
        q = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        nq = int((lab != _lib.LABEL_NONE).sum()) if q is None else len(q)
        s, other = np.empty(nq, dtype=np.float64), np.empty(nq, dtype=np.uint32)
        score, sec = C.c_double(), C.c_double()
        self._ck(self._L.f2v_silhouette(self._h, _u32(lab), nc, _u32(q) if q is not None else None, nq, s.ctypes.data_as(_lib.f64p) if samples else None,
                                        _u32(other) if samples else None, C.byref(score), C.byref(sec)))
        self.last_separation_seconds = sec.value
        return (score.value, s, other) if samples else score.value

    def davies_bouldin(self, labels, details=False):
        """The Davies-Bouldin score of `labels` in the embedding space, on the GPU -> the score, or with details=True
        (score, centroids float32[n_clusters, dim], scatter float64[n_clusters], counts uint64[n_clusters])."""
        lab, nc = self._labelling(labels)
        centroids, scatter, counts = np.empty((nc, self.dim), dtype=np.float32), np.empty(nc, dtype=np.float64), np.empty(nc, dtype=np.uint64)
        score, sec = C.c_double(), C.c_double()
        self._ck(self._L.f2v_davies_bouldin(self._h, _u32(lab), nc, C.byref(score), _f32(centroids), scatter.ctypes.data_as(_lib.f64p),
                                            counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(sec)))
        self.last_separation_seconds = sec.value
        return (score.value, centroids, scatter, counts) if details else score.value

    # -- layout (include/f2v.h: definition; functions of the matrix, d / the second matrix, k and the samples alone) ------------------
    def pca(self, d=2, details=False):
        """The projection of the matrix onto its first `d` principal components, on the GPU (the D x D eigenproblem on the host)
        -> Y float32 [n, d], or with details=True Pca(y, components float64 [d, dim], mean float64 [dim], variance float64 [d],
        info = PcaInfo(total_variance, seconds, sweeps, converged)).  `last_layout_seconds` keeps the device time."""
        y = np.empty((self.n, d), dtype=np.float32)
        comp, mean, var = np.empty((d, self.dim), dtype=np.float64), np.empty(self.dim, dtype=np.float64), np.empty(d, dtype=np.float64)
        info = _lib.PcaInfo()
        f64 = lambda a: a.ctypes.data_as(_lib.f64p)  # noqa: E731
        self._ck(self._L.f2v_pca(self._h, d, _f32(y), f64(comp), f64(mean), f64(var), C.byref(info)))
        self.last_layout_seconds = info.seconds
        return Pca(y, comp, mean, var, PcaInfo(info.total_variance, info.seconds, info.sweeps, bool(info.converged))) if details else y

    def trustworthiness(self, Y, k=5, ids=None, samples=False):
        """How well the neighbourhoods of the matrix survive in `Y` (float32 [n, d2], any layout of the same vertices), on the GPU ->
        Trust(trustworthiness, continuity, overlap, penalty_x, penalty_y, hits, seconds, samples_x, samples_y): scikit-learn's
        trustworthiness(X, Y, n_neighbors=k), the same with the roles swapped, and the mean share of common k nearest neighbours,
        over the samples `ids` (None: every vertex), each ranked against all vertices.  samples=True: samples_x / samples_y hold every
        sample's penalties (uint64 [len(ids)]), else None."""
        Y = np.ascontiguousarray(Y, dtype=np.float32)
        if Y.ndim != 2 or Y.shape[0] != self.n:
            raise ValueError("trustworthiness: Y must be [%d, d2]" % self.n)
        q = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        nq = self.n if q is None else len(q)
        px, py = (np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)) if samples else (None, None)
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None  # noqa: E731
        out = _lib.TrustInfo()
        self._ck(self._L.f2v_trustworthiness(self._h, _f32(Y), Y.shape[1], k, _u32(q) if q is not None else None, nq, u64(px), u64(py), C.byref(out)))
        self.last_layout_seconds = out.seconds
        return Trust(out.trustworthiness, out.continuity, out.overlap, out.penalty_x, out.penalty_y, out.hits, out.seconds, px, py)

    # -- t-SNE layout (include/f2v.h: definition; a function of the matrix, the sample, the parameters and P / the start where given) --
    def _tsne_sample(self, ids):
        q = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        return q, self.n if q is None else len(q)

    def tsne_affinities(self, perplexity=30, ids=None):
        """The symmetric sparse affinity matrix P of t-SNE over the rows `ids` (None: every vertex), on the GPU -> (rowptr uint32
        [m + 1], colids uint32 [nnz], values float64 [nnz]); indices are positions in `ids`, column ids ascend inside a row."""
        q, m = self._tsne_sample(ids)
        p = float(perplexity)
        cap = 2 * m * (int(min(max(3.0 * p, 1.0), float(_lib.NEAREST_MAX_K))) if p == p else 1)  # 2 m k always suffices
        rowptr, colids, values = np.empty(m + 1, dtype=np.uint32), np.empty(max(cap, 1), dtype=np.uint32), np.empty(max(cap, 1), dtype=np.float64)
        nnz, sec = C.c_uint64(), C.c_double()
        self._ck(self._L.f2v_tsne_affinities(self._h, _u32(q) if q is not None else None, m, p, _u32(rowptr), _u32(colids),
                                             values.ctypes.data_as(_lib.f64p), cap, C.byref(nnz), C.byref(sec)))
        self.last_layout_seconds = sec.value
        return rowptr, colids[: nnz.value].copy(), values[: nnz.value].copy()

    def tsne(self, d=2, perplexity=30, iters=1000, ids=None, P=None, init=None, exaggeration=12, exaggeration_iters=250, learning_rate=None,
             kl_every=0, details=False):
        """The exact t-SNE layout of the rows `ids` (None: every vertex) in d = 2 or 3 dimensions, on the GPU, deterministic -> Y float32
        [m, d], or with details=True (Y, info dict: kl, z, learning_rate, seconds, nnz, k, kl_iters uint32 [..], kl_values float64
        [..]: the divergence after every `kl_every`-th iteration).  P: (rowptr, colids, values) as tsne_affinities returns it (None:
        computed from `perplexity`); init: float64 [m, d] (None: scikit-learn's init="pca", the PCA of the whole matrix scaled to a
        standard deviation of 1e-4).  Zero for a parameter selects its default.  `last_layout_seconds` keeps the device time."""
        q, m = self._tsne_sample(ids)
        par = _lib.TsneParams(float(perplexity), float(exaggeration), float(learning_rate or 0.0), int(iters), int(exaggeration_iters), int(kl_every), 0)
        f64 = lambda a: a.ctypes.data_as(_lib.f64p)  # noqa: E731
        pr = pc = pv = y0 = None
        if P is not None:
            pr, pc, pv = (np.ascontiguousarray(P[0], dtype=np.uint32), np.ascontiguousarray(P[1], dtype=np.uint32), np.ascontiguousarray(P[2], dtype=np.float64))
            if len(pr) != m + 1 or len(pc) != len(pv) or int(pr[-1]) != len(pc):
                raise ValueError("tsne: P must be (rowptr [m + 1], colids [nnz], values [nnz])")
        if init is not None:
            y0 = np.ascontiguousarray(init, dtype=np.float64)
            if y0.shape != (m, d):
                raise ValueError("tsne: init must be [%d, %d]" % (m, d))
        y = np.empty((m, d), dtype=np.float32)
        info = _lib.TsneInfo()
        self._ck(self._L.f2v_tsne(self._h, _u32(q) if q is not None else None, m, d, C.byref(par), _u32(pr) if pr is not None else None,
                                  _u32(pc) if pc is not None else None, f64(pv) if pv is not None else None, f64(y0) if y0 is not None else None,
                                  _f32(y), C.byref(info)))
        self.last_layout_seconds = info.seconds
        if not details:
            return y
        count = C.c_uint32()
        self._ck(self._L.f2v_tsne_kl_log(self._h, None, None, 0, C.byref(count)))
        its, vals = np.zeros(max(count.value, 1), dtype=np.uint32), np.zeros(max(count.value, 1), dtype=np.float64)
        self._ck(self._L.f2v_tsne_kl_log(self._h, _u32(its), f64(vals), count.value, C.byref(count)))
        return y, dict(kl=info.kl, z=info.z, learning_rate=info.learning_rate, seconds=info.seconds, nnz=info.nnz, k=info.k,
                       kl_iters=its[: count.value], kl_values=vals[: count.value])

    # -- fold-in (include/f2v.h: definition; a function of the matrix, the lists, option, iters, ns, lr, init, seed and index_base alone) --
    def fold_in(self, rowptr, colids=None, option=5, iters=300, ns=5, lr=0.02, init="mean", seed=1, index_base=0, details=False):
        """Vectors for m new vertices whose neighbours are existing vertices, on the GPU: `iters` epochs of the option's row update
        against the matrix as it stands, every existing row held fixed -> float32 [m, dim], or with details=True (that,
        FoldInfo(seconds, pairs, resident)).  The lists are CSR-like (rowptr uint32 [m + 1], colids: 0-based ids below n, in summation
        order, duplicates kept), or `rowptr` is a list of m id lists and colids None.  init: "mean" (the neighbours' mean; a vertex
        without neighbours starts random), "random", or float32 [m, dim] of the caller's own.  Vertex q draws its negative samples as
        vertex index_base + q of `seed`: a call cut into pieces with matching index_base returns the same bits.  `last_fold_seconds`
        keeps the device time."""
        if colids is None:
            lists = [np.asarray(l, dtype=np.uint32).reshape(-1) for l in rowptr]
            rowptr = np.zeros(len(lists) + 1, dtype=np.uint32)
            if lists:
                rowptr[1:] = np.cumsum([len(l) for l in lists])
            colids = np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint32)
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint32).reshape(-1)
        colids = np.ascontiguousarray(colids, dtype=np.uint32).reshape(-1)
        if len(rowptr) < 1:
            raise ValueError("fold_in: rowptr holds m + 1 offsets")
        m = len(rowptr) - 1
        if m and len(colids) < int(rowptr[-1]):
            raise ValueError("fold_in: rowptr names %d ids, colids holds %d" % (int(rowptr[-1]), len(colids)))
        y0 = None
        if isinstance(init, str):
            if init not in FOLD_INITS:
                raise ValueError("fold_in: init must be one of %s or an array [m, dim]" % sorted(FOLD_INITS))
            kind = FOLD_INITS[init]
        else:
            y0 = np.ascontiguousarray(init, dtype=np.float32)
            if y0.shape != (m, self.dim):
                raise ValueError("fold_in: init must be [%d, %d]" % (m, self.dim))
            kind = _lib.FOLD_INIT_GIVEN
        if len(colids) == 0:
            colids = np.zeros(1, dtype=np.uint32)  # (an address for the library's null check: no id is read)
        y = np.empty((m, self.dim), dtype=np.float32)
        info = _lib.FoldInfo()
        self._ck(self._L.f2v_fold_in(self._h, option, _u32(rowptr), _u32(colids), m, iters, ns, lr, kind, _f32(y0) if y0 is not None else None,
                                     seed, index_base, _f32(y), C.byref(info)))
        self.last_fold_seconds = info.seconds
        return (y, FoldInfo(info.seconds, info.pairs, bool(info.resident))) if details else y

    # -- logistic regression (include/f2v.h: definition; a function of the matrix, the samples, the targets and the weights alone) --
    def _samples(self, ids, pairs, feature):
        """-> (a, b or None, feature code) of row samples `ids` or of `pairs` = (u, v)"""
        if (ids is None) == (pairs is None):
            raise ValueError("logreg: give either ids or pairs")
        if ids is not None:
            return np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1), None, _lib.PAIR_HADAMARD
        a = np.ascontiguousarray(pairs[0], dtype=np.uint32).reshape(-1)
        b = np.ascontiguousarray(pairs[1], dtype=np.uint32).reshape(-1)
        if len(a) != len(b):
            raise ValueError("logreg: pairs must be two arrays of one length")
        if feature not in PAIR_FEATURES:
            raise ValueError("logreg: feature must be one of %s" % sorted(PAIR_FEATURES))
        return a, b, PAIR_FEATURES[feature]

    @staticmethod
    def _targets(y, m):
        y = np.ascontiguousarray(y, dtype=np.uint8)
        y = y.reshape(m, -1) if y.ndim != 2 else y
        if y.shape[0] != m:
            raise ValueError("logreg: one row of targets per sample")
        return np.ascontiguousarray(y)

    def logreg_eval(self, weights, y, ids=None, pairs=None, feature="hadamard", lam=1.0):
        """Loss and gradient of every class at `weights` (float64 [classes, dim + 1], bias last) -> (loss [classes], grad
        [classes, dim + 1]); y: 0/1 [m, classes]."""
        a, b, code = self._samples(ids, pairs, feature)
        y = self._targets(y, len(a))
        W = np.ascontiguousarray(weights, dtype=np.float64)
        if W.shape != (y.shape[1], self.dim + 1):
            raise ValueError("logreg_eval: weights must be [%d, %d]" % (y.shape[1], self.dim + 1))
        loss, grad, sec = np.empty(len(W)), np.empty_like(W), C.c_double()
        self._ck(self._L.f2v_logreg_eval(self._h, _u32(a), _u32(b) if b is not None else None, len(a), code, y.ctypes.data_as(_lib.u8p), y.shape[1],
                                         W.ctypes.data_as(_lib.f64p), lam, loss.ctypes.data_as(_lib.f64p), grad.ctypes.data_as(_lib.f64p), C.byref(sec)))
        self.last_logreg_seconds = sec.value
        return loss, grad

    def logreg_fit(self, ids=None, pairs=None, y=None, feature="hadamard", lam=1.0, tol=1e-4, max_iter=100):
        """One-vs-rest L2-regularised logistic regression on rows `ids` or on `pairs` = (u, v) with the given pair feature, fitted by
        the L-BFGS of include/f2v.h with every pass over the samples on the GPU -> LogregModel(weights float64 [classes, dim + 1],
        feature, and per class: loss, gnorm_inf, iterations, evaluations, converged; seconds of device time)."""
        a, b, code = self._samples(ids, pairs, feature)
        y = self._targets(y, len(a))
        nc = y.shape[1]
        W = np.empty((nc, self.dim + 1), dtype=np.float64)
        info = (_lib.LogregInfo * max(nc, 1))()
        self._ck(self._L.f2v_logreg_fit(self._h, _u32(a), _u32(b) if b is not None else None, len(a), code, y.ctypes.data_as(_lib.u8p), nc, lam, tol,
                                        max_iter, W.ctypes.data_as(_lib.f64p), info))
        self.last_logreg_seconds = info[0].seconds
        col = lambda name, dtype: np.array([getattr(info[k], name) for k in range(nc)], dtype=dtype)
        return LogregModel(W, feature if b is not None else None, col("loss", np.float64), col("gnorm_inf", np.float64), col("iterations", np.uint32),
                           col("evaluations", np.uint32), col("converged", bool), info[0].seconds)

    def logreg_decision(self, model, ids=None, pairs=None):
        """The decision values z [m, classes] of `model` (a LogregModel, or weights [classes, dim + 1] with pair feature
        "hadamard") for unseen samples."""
        W, feature = (model.weights, model.feature) if isinstance(model, LogregModel) else (model, "hadamard")
        a, b, code = self._samples(ids, pairs, feature or "hadamard")
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.dim + 1:
            raise ValueError("logreg_decision: weights must be [classes, %d]" % (self.dim + 1))
        z, sec = np.empty((len(a), len(W)), dtype=np.float64), C.c_double()
        self._ck(self._L.f2v_logreg_decision(self._h, _u32(a), _u32(b) if b is not None else None, len(a), code, W.ctypes.data_as(_lib.f64p), len(W),
                                             z.ctypes.data_as(_lib.f64p), C.byref(sec)))
        self.last_logreg_seconds = sec.value
        return z

    def classify(self, labels, train_ids, test_ids, lam=1.0, tol=1e-4, max_iter=100):
        """Node classification as the reference scores it (performancescores/runnodeclassclust.py): `labels` is a list of label
        lists, one per vertex; the classes are 0 .. (number of distinct labels) - 1.  Fits on `train_ids`, predicts for every test
        vertex as many labels as it truly has -- the largest decision values, ties to the lower class -- and returns
        F1(micro, macro) in percent over all classes."""
        classes = len({v for l in labels for v in l})
        train_ids, test_ids = np.asarray(train_ids, dtype=np.uint32), np.asarray(test_ids, dtype=np.uint32)

        def onehot(ids):
            y = np.zeros((len(ids), classes), dtype=np.uint8)
            for r, v in enumerate(ids):
                y[r, [l for l in labels[v] if l < classes]] = 1
            return y

        model = self.logreg_fit(ids=train_ids, y=onehot(train_ids), lam=lam, tol=tol, max_iter=max_iter)
        z = self.logreg_decision(model, ids=test_ids)
        true = onehot(test_ids)
        order = np.argsort(-z, axis=1, kind="stable")  # descending decision value, ties to the lower class
        pred = np.zeros_like(true)
        for r in range(len(test_ids)):
            pred[r, order[r, :int(true[r].sum())]] = 1
        return _f1(true, pred, np.arange(classes))

    # -- link prediction pairs (include/f2v.h: definition; a function of the CSR, ratio and seed alone) --
    def link_pairs(self, ratio=2, seed=1, details=False):
        """The reference's link-prediction pair set (makeLinkPredictionData, performancescores/runlinkpredict.py:51-107) built on the
        GPU: every edge once as a positive, `ratio` times as many non-neighbours per vertex as negatives, shuffled by a keyed
        bijection -> (u uint32 [M], v uint32 [M], y uint8 [M]), or with details=True (u, v, y, LinkInfo(seconds, positives, negatives,
        candidates, capped)).  Needs no embeddings.  `last_link_seconds` keeps the device time."""
        count, info = C.c_uint64(), _lib.LinkInfo()
        self._ck(self._L.f2v_link_pairs(self._h, ratio, seed, None, None, None, 0, C.byref(count), C.byref(info)))
        m, seconds = count.value, info.seconds
        u, v, y = np.empty(m, dtype=np.uint32), np.empty(m, dtype=np.uint32), np.empty(m, dtype=np.uint8)
        if m:
            self._ck(self._L.f2v_link_pairs(self._h, ratio, seed, _u32(u), _u32(v), y.ctypes.data_as(_lib.u8p), m, C.byref(count), C.byref(info)))
            seconds += info.seconds
        self.last_link_seconds = seconds
        return (u, v, y, LinkInfo(seconds, info.positives, info.negatives, info.candidates, info.capped)) if details else (u, v, y)

    # -- held-out link prediction (include/f2v.h: definition) --
    def edge_split(self, frac=0.2, seed=1, ratio=1, details=False, keep="anchor"):
        """Hide a share of the edges (include/f2v.h: a keyed hash of the pair below frac, except every vertex's anchor edge) ->
        EdgeSplit(rowptr, colids: the training CSR; held_u, held_v: the hidden edges, u < v; neg_u, neg_v: `ratio` times as many
        non-edges of the full graph per vertex), with details=True also info = SplitInfo(seconds, edges, candidates_held, protected,
        held, train_nnz, negatives, drawn, capped).  A function of (CSR, frac, seed, ratio) alone; needs no embeddings.
        keep="forest" (f2v_edge_split_connected) protects the greatest spanning forest of the seed's keys instead of the anchors: the
        training graph then has exactly the components of the full graph, and no rule that keeps them hides more of the candidates.
        `last_split_seconds` keeps the device time."""
        if keep not in ("anchor", "forest"):
            raise ValueError('edge_split: keep must be "anchor" or "forest"')
        call = self._L.f2v_edge_split if keep == "anchor" else self._L.f2v_edge_split_connected
        counts, info = [C.c_uint64() for _ in range(3)], _lib.SplitInfo()
        refs = [C.byref(x) for x in counts]
        self._ck(call(self._h, frac, seed, ratio, None, None, 0, None, None, 0, None, None, 0, *refs, C.byref(info)))
        nnz, held, neg = (x.value for x in counts)
        seconds = info.seconds
        rowptr, colids = np.empty(self.n + 1, dtype=np.uint32), np.empty(nnz, dtype=np.uint32)
        hu, hv = np.empty(held, dtype=np.uint32), np.empty(held, dtype=np.uint32)
        nu, nv = np.empty(neg, dtype=np.uint32), np.empty(neg, dtype=np.uint32)
        self._ck(call(self._h, frac, seed, ratio, _u32(rowptr), _u32(colids), nnz, _u32(hu), _u32(hv), held, _u32(nu), _u32(nv), neg, *refs, C.byref(info)))
        self.last_split_seconds = seconds = seconds + info.seconds
        if not details:
            return EdgeSplit(rowptr, colids, hu, hv, nu, nv)
        return EdgeSplitDetails(rowptr, colids, hu, hv, nu, nv, SplitInfo(seconds, info.edges, info.candidates_held, info.protected_edges, info.held,
                                                                          info.train_nnz, info.negatives, info.drawn, info.capped))

    # -- components, spanning forests and subgraphs (include/f2v.h: definition; functions of the CSR, and the seed, alone) --
    def components(self, details=False):
        """The connected components of the graph (undirected, duplicates collapsed, self-loops ignored) on the GPU -> labels uint32[n],
        the smallest vertex id of each vertex's component, or with details=True (labels, Components(sizes uint32[n], components,
        isolated, largest, largest_label, edges, rounds, seconds)).  Needs no embeddings.  `last_components_seconds` keeps the
        device time."""
        labels, sizes, info = np.empty(self.n, dtype=np.uint32), np.empty(self.n, dtype=np.uint32), _lib.ComponentsInfo()
        self._ck(self._L.f2v_components(self._h, _u32(labels), _u32(sizes) if details else None, C.byref(info)))
        self.last_components_seconds = info.seconds
        if not details:
            return labels
        return labels, Components(sizes, info.components, info.isolated, info.largest, info.largest_label, info.edges, info.rounds, info.seconds)

    def spanning_forest(self, seed=1, greatest=True, details=False):
        """The spanning forest of the graph that Kruskal builds over the pairs in descending (greatest=True) or ascending order of
        (key >> (64 - "forest_key_bits"), a, b), key the pair's hash of edge_split(seed) -> (u uint32[m], v uint32[m]), u < v,
        ascending by (u, v), m = n - components; with details=True (u, v, Forest(seconds, edges, forest_edges, components, rounds,
        round_seconds)).  Needs no embeddings.  `last_forest_seconds` keeps the device time."""
        count, info = C.c_uint64(), _lib.ForestInfo()
        u, v = np.empty(max(self.n, 1) - 1, dtype=np.uint32), np.empty(max(self.n, 1) - 1, dtype=np.uint32)  # (a forest has at most n - 1 pairs)
        self._ck(self._L.f2v_spanning_forest(self._h, seed, 1 if greatest else 0, _u32(u), _u32(v), len(u), C.byref(count), C.byref(info)))
        self.last_forest_seconds = info.seconds
        u, v = u[:count.value].copy(), v[:count.value].copy()
        if not details:
            return u, v
        rounds = C.c_uint32()
        self._ck(self._L.f2v_forest_round_seconds(self._h, None, 0, C.byref(rounds)))
        per_round = np.zeros(rounds.value, dtype=np.float64)
        self._ck(self._L.f2v_forest_round_seconds(self._h, per_round.ctypes.data_as(_lib.f64p), rounds.value, C.byref(rounds)))
        return u, v, Forest(info.seconds, info.edges, info.forest_edges, info.components, info.rounds, per_round)

    def subgraph(self, keep):
        """The subgraph induced on `keep` (a boolean mask of n entries, or a list of vertex ids), relabelled by rank: ascending old id,
        ascending new id; duplicates and self-loops stay -> Subgraph(rowptr, colids, ids: the old id of each new row, new_id
        uint32[n]: the new id of each old vertex, 0xFFFFFFFF where it is dropped).  `last_subgraph_seconds` keeps the device time."""
        keep = np.asarray(keep)
        if keep.dtype == np.bool_:
            if keep.shape != (self.n,):
                raise ValueError("subgraph: a mask has one entry per vertex")
            mask = keep.astype(np.uint8)
        else:
            ids = keep.astype(np.int64).reshape(-1)
            if len(ids) and (ids.min() < 0 or ids.max() >= self.n):
                raise ValueError("subgraph: vertex id out of range")
            mask = np.zeros(self.n, dtype=np.uint8)
            mask[ids] = 1
        mask = np.ascontiguousarray(mask)
        rows, nnz = C.c_uint32(), C.c_uint64()
        self._ck(self._L.f2v_subgraph(self._h, mask.ctypes.data_as(_lib.u8p), None, None, 0, None, C.byref(rows), C.byref(nnz)))
        rowptr, colids, new_id = np.empty(rows.value + 1, dtype=np.uint32), np.empty(nnz.value, dtype=np.uint32), np.empty(self.n, dtype=np.uint32)
        self._ck(self._L.f2v_subgraph(self._h, mask.ctypes.data_as(_lib.u8p), _u32(rowptr), _u32(colids), nnz.value, _u32(new_id), C.byref(rows), C.byref(nnz)))
        self.last_subgraph_seconds = self.get_param("last_subgraph_us") * 1e-6
        return Subgraph(rowptr, colids, np.flatnonzero(mask).astype(np.uint32), new_id)

    def largest_component(self):
        """subgraph() of the largest component (ties to the lowest label) -> Subgraph."""
        labels, info = self.components(details=True)
        return self.subgraph(labels == info.largest_label)

    def pair_scores(self, u, v, metric="dot"):
        """The similarity of rows u[i] and v[i] of the matrix (metric: "dot" | "l2" | "cos", as `nearest` defines them) -> float32 [m],
        each bit-equal to the score `nearest` reports for that (query, id).  `last_pairs_seconds` keeps the device time."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32).reshape(-1), np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
        if len(u) != len(v):
            raise ValueError("pair_scores: u and v must be two arrays of one length")
        out, sec = np.empty(len(u), dtype=np.float32), C.c_double()
        self._ck(self._L.f2v_pair_scores(self._h, _u32(u), _u32(v), len(u), METRICS[metric] if isinstance(metric, str) else int(metric), _f32(out), C.byref(sec)))
        self.last_pairs_seconds = sec.value
        return out

    def ranking(self, scores, y):
        """ROC-AUC (ties count half) and average precision of `scores` against the 0/1 labels `y`, sorted and tallied on the GPU ->
        Ranking(auc, ap, concordant, tied, positives, negatives, groups, seconds); larger scores rank first, NaN last.  The result is
        a function of the multiset of (score, label): the same bits under every permutation."""
        s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.uint8).reshape(-1)
        if len(s) != len(y):
            raise ValueError("ranking: one label per score")
        r = _lib.RankingInfo()
        self._ck(self._L.f2v_ranking(self._h, s.ctypes.data_as(_lib.f64p), y.ctypes.data_as(_lib.u8p), len(s), C.byref(r)))
        return Ranking(r.auc, r.ap, r.concordant, r.tied, r.positives, r.negatives, r.groups, r.seconds)

    def heldout_scores(self, split, metric="dot", feature=None, lam=1.0, tol=1e-4, max_iter=100, ratio=2, seed=1):
        """Held-out link prediction.  Called on the engine that was built on split.rowptr / split.colids and trained there: ranks
        the split's hidden edges against its negatives by `pair_scores(metric)` -> HeldoutScores(auc, ap, classifier_auc,
        classifier_ap).  With `feature` ("hadamard" | "l1" | "l2" | "average") they are also ranked by the decision values of a
        logistic regression fitted on this engine's own link_pairs(ratio, seed) -- pairs of the training graph only; without it the
        two classifier values are None."""
        u = np.concatenate([split.held_u, split.neg_u]).astype(np.uint32)
        v = np.concatenate([split.held_v, split.neg_v]).astype(np.uint32)
        y = np.concatenate([np.ones(len(split.held_u), dtype=np.uint8), np.zeros(len(split.neg_u), dtype=np.uint8)])
        own = self.ranking(self.pair_scores(u, v, metric), y)
        if feature is None:
            return HeldoutScores(own.auc, own.ap, None, None)
        tu, tv, ty = self.link_pairs(ratio=ratio, seed=seed)
        model = self.logreg_fit(pairs=(tu, tv), y=ty.reshape(-1, 1), feature=feature, lam=lam, tol=tol, max_iter=max_iter)
        clf = self.ranking(self.logreg_decision(model, pairs=(u, v))[:, 0], y)
        return HeldoutScores(own.auc, own.ap, clf.auc, clf.ap)

    # -- neighbourhood scores of pairs (include/f2v.h: definition; a function of the CSR, the pair and the kinds alone) --
    def pair_neighbourhood(self, u, v, kinds=("cn", "jaccard", "aa", "ra", "pa")):
        """The classic neighbourhood scores of the pairs (u[i], v[i]) on this engine's graph, on the GPU -> dict of name -> float64
        [m] for the names in `kinds`: "cn" common neighbours, "jaccard", "aa" Adamic-Adar, "ra" resource allocation, "pa"
        preferential attachment.  Needs no embeddings.  `last_neighbourhood_seconds` keeps the device time."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32).reshape(-1), np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
        if len(u) != len(v):
            raise ValueError("pair_neighbourhood: u and v must be two arrays of one length")
        names = [kinds] if isinstance(kinds, str) else list(kinds)
        unknown = [k for k in names if k not in NEIGHBOURHOOD_KINDS]
        if unknown or not names:
            raise ValueError("pair_neighbourhood: kinds are taken from %s" % ", ".join(NEIGHBOURHOOD_KINDS))
        mask = 0
        for k in names:
            mask |= NEIGHBOURHOOD_KINDS[k]
        asked = [k for k, bit in NEIGHBOURHOOD_KINDS.items() if mask & bit]  # ascending bit: the layout of the result
        out, sec = np.empty((len(asked), len(u)), dtype=np.float64), C.c_double()
        self._ck(self._L.f2v_pair_neighbourhood(self._h, _u32(u), _u32(v), len(u), mask, out.ctypes.data_as(_lib.f64p), C.byref(sec)))
        self.last_neighbourhood_seconds = sec.value
        return {k: out[asked.index(k)] for k in names}

    def heldout_baselines(self, split, kinds=("cn", "jaccard", "aa", "ra", "pa")):
        """The yardstick of `heldout_scores`.  Called on the engine that was built on split.rowptr / split.colids: scores the split's
        hidden edges and its negatives by `pair_neighbourhood(kinds)` on the training graph and ranks each kind with `ranking`
        -> dict of name -> Ranking.  Needs no embeddings."""
        u = np.concatenate([split.held_u, split.neg_u]).astype(np.uint32)
        v = np.concatenate([split.held_v, split.neg_v]).astype(np.uint32)
        y = np.concatenate([np.ones(len(split.held_u), dtype=np.uint8), np.zeros(len(split.neg_u), dtype=np.uint8)])
        return {k: self.ranking(s, y) for k, s in self.pair_neighbourhood(u, v, kinds).items()}

    # -- ranks of pairs (include/f2v.h: definition; two integers per pair, a function of the matrix, the CSR, the pair, metric and flags) --
    def pair_ranks(self, u, v, metric="dot", exclude_self=True, exclude_neighbours=True, ks=(1, 10, 50, 100)):
        """Where v[i] stands among all vertices ordered by similarity to u[i] (metric as `nearest` defines it), with u[i] itself and
        its neighbours in this engine's graph left out of the candidates -> PairRanks(greater uint32[m], equal uint32[m]: the
        candidates that rank above v[i] / tie with it; mrr and mean_rank of the mid-ranks 1 + greater + equal / 2; hits: dict K ->
        the number of pairs with mid-rank <= K; candidates: the sum of the candidate counts; tied_pairs; seconds).  Counted over all n
        rows on the GPU: no top-k, no limit on the rank.  `last_ranks_seconds` keeps the device time."""
        u, v = np.ascontiguousarray(u, dtype=np.uint32).reshape(-1), np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
        if len(u) != len(v):
            raise ValueError("pair_ranks: u and v must be two arrays of one length")
        kk = np.ascontiguousarray(list(ks), dtype=np.uint32)
        flags = (_lib.NEAREST_EXCLUDE_SELF if exclude_self else 0) | (_lib.NEAREST_EXCLUDE_NEIGHBOURS if exclude_neighbours else 0)
        greater, equal = np.empty(len(u), dtype=np.uint32), np.empty(len(u), dtype=np.uint32)
        hits, info = np.zeros(len(kk), dtype=np.uint64), _lib.PairRanksInfo()
        self._ck(self._L.f2v_pair_ranks(self._h, _u32(u), _u32(v), len(u), METRICS[metric] if isinstance(metric, str) else int(metric), flags,
                                        _u32(greater), _u32(equal), _u32(kk) if len(kk) else None, len(kk),
                                        hits.ctypes.data_as(C.POINTER(C.c_uint64)) if len(kk) else None, C.byref(info)))
        self.last_ranks_seconds = info.seconds
        return PairRanks(greater, equal, info.mrr, info.mean_rank, {int(k): int(h) for k, h in zip(kk, hits)}, info.candidates, info.tied_pairs, info.seconds)

    def heldout_ranks(self, split, metric="dot", sample=None, both_ends=True, ks=(1, 10, 50, 100)):
        """The filtered ranks of a split's hidden edges.  Called on the engine that was built on split.rowptr / split.colids and trained
        there: `pair_ranks` of the hidden edges with both exclusions set, so that a vertex's training edges are no rivals of its hidden
        one -> PairRanks.  With H hidden edges and 0 < sample < H the edges ranked are those of index floor(j H / sample), j < sample
        (no random numbers; the held list is ordered by u, so the stride spreads over the vertices).  Each chosen edge {a, b} gives the
        pair (a, b) and, with `both_ends`, (b, a) behind it."""
        hu, hv = np.asarray(split.held_u, dtype=np.uint32), np.asarray(split.held_v, dtype=np.uint32)
        H = len(hu)
        if sample is not None and 0 < int(sample) < H:
            pick = [j * H // int(sample) for j in range(int(sample))]  # (Python integers: no overflow)
            hu, hv = hu[pick], hv[pick]
        if both_ends:
            u, v = np.stack([hu, hv], axis=1).reshape(-1), np.stack([hv, hu], axis=1).reshape(-1)
        else:
            u, v = hu, hv
        return self.pair_ranks(u, v, metric, True, True, ks)

    # -- communities (include/f2v.h: definition; a function of the CSR, seed, max_levels and max_sweeps alone) --
    def communities(self, seed=1, max_levels=32, max_sweeps=64, details=False):
        """The communities of the graph itself (Louvain, in integers: bit-reproducible), on the GPU -> labels uint32[n], or with
        details=True (labels, Communities(modularity, communities, levels, edges, seconds, level_records, level_labels uint32[levels,
        n])); level_records: LouvainLevel(nodes, communities, sweeps, moves, qnum) per level.  `modularity` equals
        `modularity(labels).q`.  Needs no embeddings.  `last_louvain_seconds` keeps the device time."""
        max_levels, max_sweeps = int(max_levels), int(max_sweeps)
        if not 0 <= max_levels < 2 ** 16:
            raise ValueError("communities: max_levels must be below 65536")
        labels = np.empty(self.n, dtype=np.uint32)
        per_level = np.empty((max_levels, self.n), dtype=np.uint32) if details else None
        records, info = (_lib.LouvainLevel * max(max_levels, 1))(), _lib.LouvainInfo()
        self._ck(self._L.f2v_louvain(self._h, seed, max_levels, max_sweeps, _u32(labels), _u32(per_level) if details else None, records, C.byref(info)))
        self.last_louvain_seconds = info.seconds
        if not details:
            return labels
        recs = [LouvainLevel(r.nodes, r.communities, r.sweeps, r.moves, r.qnum) for r in records[:info.levels]]
        return labels, Communities(info.modularity, info.communities, info.levels, info.edges, info.seconds, recs, per_level[:info.levels].copy())

    def agreement(self, a, b):
        """How far two labellings agree (any integer arrays, one label per vertex; negative = the vertex takes no part), the
        contingency table counted on the GPU -> Agreement(nmi, ari, mi, entropy_a, entropy_b, n, sum_comb, sum_a, sum_b, total, rows,
        cols, seconds): normalised mutual information (arithmetic mean of the entropies), adjusted Rand index, and their integers."""
        (la, ka), (lb, kb) = self._labelling(a), self._labelling(b)
        info = _lib.AgreementInfo()
        self._ck(self._L.f2v_partition_agreement(self._h, _u32(la), ka, _u32(lb), kb, C.byref(info)))
        return Agreement(info.nmi, info.ari, info.mi, info.entropy_a, info.entropy_b, info.n, info.sum_comb, info.sum_a, info.sum_b, info.total,
                         info.rows, info.cols, info.seconds)

    def link_predict(self, u=None, v=None, y=None, train_frac=0.5, feature="hadamard", lam=1.0, tol=1e-4, max_iter=100, ratio=2, seed=1):
        """Link prediction as the reference scores it (performancescores/runlinkpredict.py:127-140): fits on the first
        int(m * train_frac) pairs (u, v) with 0/1 targets y, predicts z > 0 on the rest -> LinkScores(accuracy, f1_macro, f1_micro)
        in percent, the F1 values over the labels that occur among the predictions.  Without u, v and y the pair set is
        link_pairs(ratio, seed)."""
        given = [x is not None for x in (u, v, y)]
        if any(given) and not all(given):
            raise ValueError("link_predict: give u, v and y together, or none of them")
        if not any(given):
            u, v, y = self.link_pairs(ratio=ratio, seed=seed)
        u, v, y = np.asarray(u, dtype=np.uint32), np.asarray(v, dtype=np.uint32), np.asarray(y, dtype=np.uint8).reshape(-1)
        cv = int(len(y) * train_frac)
        model = self.logreg_fit(pairs=(u[:cv], v[:cv]), y=y[:cv].reshape(-1, 1), feature=feature, lam=lam, tol=tol, max_iter=max_iter)
        pred = (self.logreg_decision(model, pairs=(u[cv:], v[cv:]))[:, 0] > 0).astype(np.uint8)
        true = y[cv:]
        two = lambda a: np.stack([a == 0, a == 1], axis=1)
        f1 = _f1(two(true), two(pred), np.unique(pred))
        return LinkScores(100.0 * float((pred == true).mean()) if len(true) else 0.0, f1.macro, f1.micro)

    def stats(self):
        s = _lib.Stats()
        self._ck(self._L.f2v_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}


def shard_bounds_balanced(rowptr, lo, hi, world):
    """f2v_shard_bounds (host only): uint32[world+1], slice r = rows [b[r], b[r+1]) of minibatch [lo,hi), balanced by degree + 4."""
    rp = np.ascontiguousarray(rowptr, dtype=np.uint32)
    out = np.zeros(world + 1, dtype=np.uint32)
    check(_lib.lib().f2v_shard_bounds(_u32(rp), lo, hi, world, _u32(out)))
    return out


def push_masks(rowptr, colids, batch, world, sample_ids=()):
    """f2v_push_masks (host only): uint32[n], bit r = rank r reads the row without owning it."""
    rp = np.ascontiguousarray(rowptr, dtype=np.uint32)
    ci = np.ascontiguousarray(colids, dtype=np.uint32)
    ids = np.ascontiguousarray(sample_ids, dtype=np.uint32)
    out = np.zeros(len(rp) - 1, dtype=np.uint32)
    check(_lib.lib().f2v_push_masks(_u32(rp), _u32(ci), len(rp) - 1, batch, world, _u32(ids), len(ids), _u32(out)))
    return out


def write_embd(path, X):
    X = np.ascontiguousarray(X, dtype=np.float32)
    check(_lib.lib().f2v_write_embd(str(path).encode(), _f32(X), X.shape[0], X.shape[1]))


def write_embd_bin(path, X):
    """Raw fp32 N x D file (the scorers' readBinEmbeddings format, runnodeclassclust.py:81-100)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    check(_lib.lib().f2v_write_embd_bin(str(path).encode(), _f32(X), X.shape[0], X.shape[1]))


def read_embd(path):
    """Text .embd (writeToFile's format) -> float32 [N, D]."""
    L = _lib.lib()
    n, d, x = C.c_uint32(), C.c_uint32(), _lib.f32p()
    check(L.f2v_read_embd(str(path).encode(), C.byref(n), C.byref(d), C.byref(x)))
    try:
        return np.ctypeslib.as_array(x, shape=(n.value, d.value)).copy()
    finally:
        L.f2v_free(x)


def read_embd_bin(path, n, dim):
    """Raw fp32 N x D file (write_embd_bin) -> float32 [N, D]."""
    X = np.empty((n, dim), dtype=np.float32)
    check(_lib.lib().f2v_read_embd_bin(str(path).encode(), n, dim, _f32(X)))
    return X


def output_name(input_path, outdir, option, bs_mode, batch, dim, iters, ns):
    buf = C.create_string_buffer(4096)
    check(_lib.lib().f2v_output_name(str(input_path).encode(), str(outdir).encode(), option, bs_mode, batch, dim, iters, ns, buf, len(buf)))
    return buf.value.decode()


def sm_table():
    t = np.empty(2048, dtype=np.float32)
    check(_lib.lib().f2v_sm_table(_f32(t)))
    return t


class algorithms:
    """Mirror of `class algorithms` (sample/algorithms.h:51-137) on the GPU engine."""

    def __init__(self, graph, input_path="", outputdir="", dim=128, gamma=1.0, bsize=384, device=0):
        rowptr, colids = graph
        self.engine = Engine(rowptr, colids, dim, device)
        self.DIM = dim
        self.filename = input_path
        self.outputdir = outputdir
        self.gpu_train_seconds = 0.0
        self.nCoordinates = None  # filled after a run (host copy of the HBM matrix)

    def srand(self, seed=1):  # Test/Force2Vec.cpp:126
        self.engine.srand(seed)

    def _run(self, option, bs, ITER, BATCH, ns, lr, write=True):
        t0 = time.perf_counter()
        self.engine.init_embeddings(INIT_SYMMETRIC if option in (1, 5, 8, 11) else INIT_UNIT)
        self.gpu_train_seconds = self.engine.train(option, ITER, BATCH, ns, lr, bs)
        sec = time.perf_counter() - t0
        self.nCoordinates = self.engine.get_embeddings()
        if write and self.filename:
            self.writeToFile(output_name(self.filename, self.outputdir, option, bs, BATCH, self.DIM, ITER, ns))
        return [sec]

    def AlgoForce2Vec(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE):
        """Option 1, the exact all-pairs Force2Vec (sample/algorithms.cpp:344-445): no samples, no learning rate."""
        return self._run(1, 0, ITERATIONS, BATCHSIZE, 0, 0.0)

    def AlgoForce2VecNS(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(5, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSBS(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(5, 1, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSRW(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(6, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSRWBS(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(6, 1, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSRWEFF(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(7, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNS_SREAL_D128_AVXZ(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(8, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSRW_SREAL_D128_AVXZ(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(9, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSRWEFF_SREAL_D128_AVXZ(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(10, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def AlgoForce2VecNSLB_SREAL_D128_AVXZ(self, ITERATIONS, NUMOFTHREADS, BATCHSIZE, ns, lr):
        return self._run(11, 0, ITERATIONS, BATCHSIZE, ns, lr)

    def writeToFile(self, path):
        print("Creating output file in following directory:" + path)
        write_embd(path, self.nCoordinates)
        self.last_output = path
