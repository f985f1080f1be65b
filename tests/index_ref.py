"""A numpy restatement of "nearest neighbours through an index" (include/f2v.h), on top of nearest_ref: the probed lists are the top-P
of the exact order over the centroid matrix, the candidates are the members of those lists, the result is the exact order over the
candidates' scores with their original ids."""
import numpy as np

import nearest_ref as R


def index_ref(X, labels, centroids, k, metric, nprobe, qids=None, vectors=None, rowptr=None, colids=None, exclude_self=False, exclude_neighbours=False,
              S=None, SC=None):
    """-> (ids uint32 [nq, k], scores float32 [nq, k], probes uint32 [nq, P], candidates int).  `S`, `SC`: the queries' scores against
    the rows and against the centroids where the caller has them already (R.scores of the same arguments)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    labels = np.asarray(labels)
    centroids = np.ascontiguousarray(centroids, dtype=np.float32)
    Q = X[qids] if vectors is None else np.ascontiguousarray(vectors, dtype=np.float32)
    SC = R.scores(Q, centroids, metric) if SC is None else SC
    S = R.scores(Q, X, metric) if S is None else S
    pr = R.top_k(SC, min(nprobe, centroids.shape[0]))[0]
    out = np.ones(S.shape, dtype=bool)  # everything but the members of the probed lists is left out
    candidates = 0
    for q in range(len(Q)):
        member = np.isin(labels, pr[q])
        candidates += int(member.sum())
        out[q] = ~member
    if qids is not None and (exclude_self or exclude_neighbours):
        out |= R.exclusion_mask(qids, X.shape[0], rowptr, colids, exclude_self, exclude_neighbours)
    ids, scores = R.top_k(S, k, out)
    return ids, scores, pr, candidates
