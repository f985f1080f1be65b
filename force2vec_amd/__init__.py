"""force2vec_amd -- MI355X (gfx950) Force2Vec embedding engine.

csrc/ holds the HIP kernels and the C ABI (libf2v.so, include/f2v.h); this package is the
host-side mirror of the reference's interface for the one hot path (options 5-11 force
kernels + SGD row update).  Importing it never imports anything from oracle/.

Training progress: `Engine.objective(option, ns=5)` evaluates the training objective (the
reference's per-epoch loglike, defined in include/f2v.h) of the current matrix on the GPU;
with `Engine.set_param("loss_every", k)` every f2v_train logs it after every k-th epoch and
its last, read back with `Engine.train_losses()`.

Queries: `Engine.nearest(ids=..., k=10, metric="dot" | "l2" | "cos")` returns the k most similar rows of
the matrix for each query (rows or caller-supplied vectors) without the matrix leaving the GPU;
`Engine.neighbour_recall(k, metric)` is the graph-reconstruction precision@k.

Exact all-pairs Force2Vec: `Engine.train(1, iters, batch)` / `algorithms.AlgoForce2Vec` run the reference's option 1, where every vertex
is repelled by every other one (no samples, no learning rate), and `Engine.objective(1)` is its exact objective (include/f2v.h).

Clustering: `Engine.kmeans(k, max_iters=300, seed=1, restarts=1)` runs Lloyd's k-means on the rows of the matrix on the GPU
(deterministic: include/f2v.h), `Engine.modularity(labels)` scores a labelling on the input graph.

Scoring with labels: `Engine.classify(labels, train_ids, test_ids)` (node-classification F1) and `Engine.link_predict(u, v, y)` fit a
one-vs-rest logistic regression on rows or pair features with every pass over the samples on the GPU (`Engine.logreg_fit`,
`logreg_eval`, `logreg_decision`; definition in include/f2v.h).

Looking at it: `Engine.pca(d=2)` is the principal-component projection of the matrix (deterministic, include/f2v.h) and
`Engine.trustworthiness(Y, k=5)` scores any second matrix over the same vertices against it: scikit-learn's trustworthiness, its mirror
image continuity, and the overlap of the two neighbourhoods.

Vertices that arrive after training: `Engine.fold_in(rowptr, colids, option=5, iters=300)` returns their vectors -- the training rule run
for each new vertex against the frozen matrix, all epochs in one launch (deterministic, include/f2v.h) -- without training again.

Link prediction: `Engine.link_pairs(ratio=2, seed=1)` builds the reference's pair set on the GPU (every edge once, twice as many
non-neighbours per vertex, shuffled; deterministic, include/f2v.h) and `Engine.link_predict()` scores the embedding on it.

Held-out link prediction: `Engine.edge_split(frac=0.2)` hides a share of the edges (and draws as many non-edges), an engine built on
the returned training CSR is trained as usual, and its `heldout_scores(split)` ranks the hidden edges against the non-edges by the
embedding's own similarity (`Engine.pair_scores`) -> ROC-AUC and average precision (`Engine.ranking`, sorted and tallied on the GPU).
The yardstick beside it: `heldout_baselines(split)` ranks the same pairs by the classic neighbourhood scores of the training graph --
common neighbours, Jaccard, Adamic-Adar, resource allocation, preferential attachment (`Engine.pair_neighbourhood`, on the GPU).
The harder question: `heldout_ranks(split)` places every hidden edge (u, v) among ALL vertices ordered by similarity to u, the training
edges of u filtered out -> MRR, mean rank and Hits@K (`Engine.pair_ranks`: two exact counts per pair, no top-k, no limit on the rank).

What the graph itself achieves: `Engine.communities()` finds the graph's communities with the Louvain method on the GPU (integers only:
the same labels on every run; `details=True` adds their modularity, the yardstick for `modularity(kmeans(k).labels)`), and
`Engine.agreement(a, b)` gives NMI and ARI of two labellings -- clusters against communities, either against ground truth.

What the graph is made of: `Engine.components()` labels the connected components (the smallest id of each), `Engine.spanning_forest(seed)`
is the unique spanning forest of a keyed order on the edges, `Engine.edge_split(..., keep="forest")` hides edges without ever cutting a
component, and `Engine.subgraph(keep)` / `Engine.largest_component()` return an induced subgraph, relabelled, to build an engine on."""
from . import _lib  # noqa: F401
from ._lib import F2VError  # noqa: F401
from ._lib import KMEANS_MAX_K, KMEANS_PIECE  # noqa: F401
from ._lib import INDEX_MAX_LISTS, INDEX_MAX_PROBES  # noqa: F401
from ._lib import LABEL_NONE, SEPARATION_MAX_CLUSTERS, SEPARATION_PIECE, SEPARATION_SPAN  # noqa: F401
from ._lib import PCA_PIECE, TRUST_MAX_DIM, TSNE_PIECE, TSNE_SPAN  # noqa: F401
from ._lib import FOLD_INIT_GIVEN, FOLD_INIT_MEAN, FOLD_INIT_RANDOM  # noqa: F401
from ._lib import LOGREG_BLOCK, LOGREG_MAX_CLASSES, PAIR_AVERAGE, PAIR_HADAMARD, PAIR_L1, PAIR_L2  # noqa: F401
from ._lib import NEAREST_EXCLUDE_NEIGHBOURS, NEAREST_EXCLUDE_SELF, NEAREST_MAX_K, NEAREST_PAD_ID, SIM_COSINE, SIM_DOT, SIM_L2  # noqa: F401
from .engine import FoldInfo, LinkInfo, Pca, Trust  # noqa: F401
from .engine import EdgeSplit, HeldoutScores, PairRanks, Ranking, SplitInfo  # noqa: F401
from .engine import Agreement, Communities, LouvainLevel  # noqa: F401
from .engine import Components, Forest, Subgraph  # noqa: F401
from .engine import Engine, KMeans, LogregModel, Modularity, algorithms, output_name, push_masks, read_embd, read_embd_bin, sm_table, write_embd, write_embd_bin  # noqa: F401
from .graph import read_csr_bin, read_mtx, rmat_csr, write_csr_bin  # noqa: F401

__all__ = ["Engine", "F2VError", "KMeans", "LogregModel", "Modularity", "algorithms", "read_mtx", "rmat_csr", "write_embd", "output_name", "sm_table"]
