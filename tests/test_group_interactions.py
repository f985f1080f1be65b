"""-m gpu: a group's interactions in the step kernel's plain-launch form (f2v_minibatch_step: qstep_kernel), bit for bit against the
CPU oracle's ORDER_TREE.  The kernel evaluates the coefficients of a group's rows -- and of the samples staged in LDS -- once, on
the lanes of an item, and hands them round by DPP; these cases aim at what that can get wrong: items of different lengths in one
wavefront (a partly filled last group, an empty list beside full ones), hub pieces, every width and option of the kernel's forms
(the ones that keep one evaluation per row included), every way the samples arrive, partly live wavefronts, and the values whose
coefficient is inf or NaN."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 230
DEGREES = (4, 0, 8, 3, 9, 1, 7, 2, 5)  # by vertex, cyclically: a wavefront takes the items of a minibatch four at a time, longest first
HUBS = ((5, 40), (N - 3, 90))
# minibatches: (4, 0, 8, 3) -- an empty list beside full groups; (9, 1, 7, 2, 5) -- one item left over; a single row; 6 rows; then
# several workgroups' worth, 63 and 64 rows, and the ragged rest
CUTS = (0, 4, 9, 10, 16, 79, 143, N)
EQUAL = (20, 21)  # row 21 is a neighbour of row 20 and holds the same embedding: a = 0 on the attraction side
HUGE = 30         # a row of magnitude 3e19: every a with it overflows to inf


@pytest.fixture(scope="module")
def F():
    import force2vec_amd as F
    return F


@pytest.fixture(scope="module")
def graph():
    rng = np.random.default_rng(11)
    lists = []
    for v in range(N):
        d = dict(HUBS).get(v, DEGREES[v % len(DEGREES)])
        nb = rng.choice(N - 1, d, replace=False)
        nb = np.sort(nb + (nb >= v))  # (no self loops)
        lists.append(nb)
    lists[EQUAL[0]][0] = EQUAL[1]
    lists[11][0] = HUGE  # (degree 8: the huge row inside a full group)
    rowptr = np.zeros(N + 1, dtype=np.uint32)
    rowptr[1:] = np.cumsum([len(l) for l in lists])
    deg = np.diff(rowptr.astype(np.int64))
    assert set(DEGREES) | {40, 90} == set(deg.tolist())
    return rowptr, np.concatenate(lists).astype(np.uint32)


CASES = [
    # option, dim, ns, bs, chunk
    (5, 128, 5, 0, 512), (5, 128, 5, 0, 8), (5, 128, 0, 0, 8), (5, 128, 9, 0, 8), (5, 128, 5, 1, 8),
    (5, 100, 5, 0, 8), (5, 100, 9, 0, 512),
    (5, 64, 5, 0, 8), (5, 64, 9, 0, 512), (5, 64, 5, 1, 8),
    (5, 32, 5, 0, 8), (5, 32, 9, 0, 512), (5, 32, 0, 0, 8),
    (5, 16, 5, 0, 8), (5, 16, 9, 0, 512),
    (6, 128, 5, 0, 8), (6, 128, 9, 0, 512), (6, 100, 5, 0, 8), (6, 100, 5, 1, 512),
]


@pytest.mark.parametrize("option,dim,ns,bs,chunk", CASES)
def test_group_interactions_bit_exact(F, graph, option, dim, ns, bs, chunk):
    rowptr, colids = graph
    rng = np.random.default_rng(100 * option + dim)
    X0 = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    X0[EQUAL[1]] = X0[EQUAL[0]]
    if option == 5:  # (the sigmoid kernel's dot products with such a row are inf - inf: nothing this change touches)
        X0[HUGE] = np.float32(3e19) * np.sign(X0[HUGE])
    eng = F.Engine(rowptr, colids, dim)
    eng.set_param("hub_chunk", chunk)
    eng.set_embeddings(X0)
    Xo = X0.copy()
    lr = 0.02
    for epoch in range(2):
        for lo, hi in zip(CUTS[:-1], CUTS[1:]):
            nid = (hi - lo) + ns - 1 if bs else ns
            ids = rng.integers(0, N - 1, max(nid, 1)).astype(np.uint32)
            if ns:
                ids[0] = lo              # the row itself: a = 0 on the repulsion side -- inf, NaN, the -5 path
                if ns > 2:
                    ids[2] = HUGE        # a = inf on the repulsion side
                if lo > 0:
                    ids[1] = lo - 1      # a row the previous minibatch has just written
            eng.minibatch_step(option, lo, hi, ids, ns, lr, bs)
            O.minibatch(option, rowptr, colids, Xo, lo, hi, ids, ns, lr, bs_mode=bs, order=O.ORDER_TREE, chunk=chunk)
    got = eng.get_embeddings()
    eng.close()
    same = (got == Xo) | (np.isnan(got) & np.isnan(Xo))
    assert same.all(), "rows that differ: %s" % np.flatnonzero(~same.all(axis=1))[:16]
    assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], Xo.view(np.uint32)[~np.isnan(Xo)])


def test_interaction_stub_hook(F, graph):
    """f2v_test_interaction_stub (self-test build; tools/interaction_stub_probe.py times launches with it): with the stub on a step
    computes something else -- the rows are gathered and added --, and switched off again the same engine is bit-exact."""
    from force2vec_amd import _lib
    rowptr, colids = graph
    dim, ns, lr = 128, 5, 0.02
    rng = np.random.default_rng(5)
    X0 = rng.uniform(-1, 1, (N, dim)).astype(np.float32)
    ids = rng.integers(0, N - 1, ns).astype(np.uint32)
    want = X0.copy()
    O.minibatch(5, rowptr, colids, want, 0, N, ids, ns, lr, order=O.ORDER_TREE, chunk=8)
    T = _lib.selftest_lib()
    eng = F.Engine(rowptr, colids, dim, selftest=True)
    eng.set_param("hub_chunk", 8)
    assert T.f2v_test_interaction_stub(None, 1) != 0  # a null handle is refused
    for mode, exact in ((3, False), (1, False), (0, True)):
        eng.set_embeddings(X0)
        _lib.check(T.f2v_test_interaction_stub(eng._h, mode), T)
        eng.minibatch_step(5, 0, N, ids, ns, lr, 0)
        assert np.array_equal(eng.get_embeddings(), want) == exact, mode
    eng.close()
