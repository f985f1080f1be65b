"""TEST INFRASTRUCTURE: the plain Python restatement of f2v_pair_neighbourhood (include/f2v.h: neighbourhood scores of pairs), written
from the header's text: N(u) and d(u), S and L, the members of W among the nonzeros of S's stored row, the two sums in the definition's
order (inside a piece of 1024 nonzeros sequentially from +0, the piece sums sequentially from +0) and the five scores.  Python floats
are fp64 and every operation below is one rounding.  Nothing here knows how the kernels place pairs, pieces of work or launches."""
import numpy as np

from exact_ref import flog
from linkpairs_ref import neighbours

PIECE = 1024
KINDS = ("cn", "jaccard", "aa", "ra", "pa")  # ascending bit: F2V_NB_COMMON .. F2V_NB_PREFERENTIAL
BITS = dict(zip(KINDS, (1, 2, 4, 8, 16)))


class Graph:
    """what the definition derives from a CSR once: d(u), and the two terms a common neighbour w adds (0 where it adds nothing)"""

    def __init__(self, rowptr, colids):
        self.rowptr, self.colids = np.asarray(rowptr, dtype=np.int64), np.asarray(colids, dtype=np.int64)
        self.n = len(self.rowptr) - 1
        self.deg = np.array([len(neighbours(self.rowptr, self.colids, u)) for u in range(self.n)], dtype=np.int64)
        d = self.deg.astype(np.float64)
        self.aa = np.where(self.deg >= 2, 1.0 / flog(np.maximum(d, 2.0)), 0.0).tolist()
        self.ra = np.where(self.deg >= 1, 1.0 / np.maximum(d, 1.0), 0.0).tolist()
        self._rows = {}

    def row(self, u):
        """(the stored row as a list, the set of its ids)"""
        if u not in self._rows:
            r = self.colids[self.rowptr[u]:self.rowptr[u + 1]].tolist()
            self._rows[u] = (r, set(r))
        return self._rows[u]

    def s_and_l(self, u, v):
        lu, lv = self.rowptr[u + 1] - self.rowptr[u], self.rowptr[v + 1] - self.rowptr[v]
        return (v, u) if lv < lu or (lv == lu and v < u) else (u, v)

    def pair(self, u, v, piece=PIECE):
        """-> (c, jaccard, aa, ra, pa) of the pair"""
        u, v = int(u), int(v)
        S, L = self.s_and_l(u, v)
        row, in_l = self.row(S)[0], self.row(L)[1]
        c, aa, ra = 0, 0.0, 0.0
        for p0 in range(0, len(row), piece):
            paa, pra = 0.0, 0.0
            for q in range(p0, min(p0 + piece, len(row))):
                w = row[q]
                if (q > 0 and row[q - 1] == w) or w == u or w == v or w not in in_l:
                    continue
                c += 1
                if self.deg[w] >= 2:
                    paa = paa + self.aa[w]
                if self.deg[w] >= 1:
                    pra = pra + self.ra[w]
            aa, ra = aa + paa, ra + pra
        du, dv = int(self.deg[u]), int(self.deg[v])
        den = du + dv - c
        return c, (float(c) / float(den) if den else 0.0), aa, ra, float(du) * float(dv)

    def scores(self, u, v, piece=PIECE):
        """-> dict of kind -> float64 [m]"""
        out = np.array([self.pair(a, b, piece) for a, b in zip(u, v)], dtype=np.float64).reshape(-1, 5)
        return {k: np.ascontiguousarray(out[:, i]) for i, k in enumerate(KINDS)}


def scores(rowptr, colids, u, v):
    return Graph(rowptr, colids).scores(u, v)
