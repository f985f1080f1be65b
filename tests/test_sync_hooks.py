"""-m gpu: the two look-inside hooks of the self-test build that only tools/ used so far -- f2v_test_stamps (tools/chain_hops.py) and
f2v_test_chain_nowait (tools/chain_probe*.py) -- on the chained launches they instrument: cora, D = 128, batch 256, hub chunk 4 (split
rows and combine trees exist), two epochs, in the chain form ("chain_wide" = 0) and in the wide form."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_graph_path

pytestmark = pytest.mark.gpu

DIM, BATCH, CHUNK, EPOCHS = 128, 256, 4, 2
FORMS = [(0, 1), (1, 2)]  # "chain_wide" -> "last_train_form"


@pytest.fixture(scope="module")
def F():
    import force2vec_amd as F
    return F


@pytest.fixture(scope="module")
def cora(F):
    return F.read_mtx(golden_graph_path("cora.mtx"))


def engine(F, cora, wide):
    eng = F.Engine(cora[0], cora[1], DIM, selftest=True)
    eng.set_param("hub_chunk", CHUNK)
    eng.set_param("chain_wide", wide)
    return eng


_fresh = {}


def fresh(F, cora, option, wide, form):
    """-> (start, result as uint32) of a fresh handle that trains without any hook; computed once per case, never changed"""
    if (option, wide) not in _fresh:
        eng = engine(F, cora, wide)
        eng.srand(1)
        eng.init_embeddings(0 if option == 5 else 1)
        X0 = eng.get_embeddings()
        eng.srand(1)
        eng.train(option, EPOCHS, BATCH)
        assert eng.get_param("last_train_form") == form
        X = eng.get_embeddings().view(np.uint32)
        eng.close()
        X0.setflags(write=False)
        X.setflags(write=False)
        _fresh[(option, wide)] = (X0, X)
    return _fresh[(option, wide)]


@pytest.mark.parametrize("wide,form", FORMS)
@pytest.mark.parametrize("option", [5, 6])
def test_stamps(F, cora, option, wide, form):
    """Per-row time stamps: they change no bit of the result; word 2 (the row's flag stored) is set for every row, word 0 (its last
    piece announced) for exactly the rows that are split (more than `hub_chunk` neighbours) -- in both forms --, and a row's last
    piece is announced before its flag is stored; reading stamps that are switched off is refused."""
    from force2vec_amd import _lib
    T = _lib.selftest_lib()
    rowptr = cora[0]
    n = len(rowptr) - 1
    X0, want = fresh(F, cora, option, wide, form)
    eng = engine(F, cora, wide)
    try:
        _lib.check(T.f2v_test_stamps(eng._h, 1, None), T)
        eng.set_embeddings(X0)
        eng.srand(1)
        eng.train(option, EPOCHS, BATCH)
        assert eng.get_param("last_train_form") == form
        st = np.zeros(4 * n, dtype=np.uint64)
        _lib.check(T.f2v_test_stamps(eng._h, 0, st.ctypes.data_as(C.POINTER(C.c_uint64))), T)
        assert np.array_equal(eng.get_embeddings().view(np.uint32), want)
        st = st.reshape(n, 4)
        deg = np.diff(rowptr.astype(np.int64))
        assert (st[:, 2] != 0).all()
        assert np.array_equal(st[:, 0] != 0, deg > CHUNK)
        both = (st[:, 0] != 0) & (st[:, 2] != 0)
        assert both.any() and (st[both, 0] <= st[both, 2]).all()
        assert T.f2v_test_stamps(eng._h, 0, st.ctypes.data_as(C.POINTER(C.c_uint64))) == _lib.F2V_ESTATE  # switched off above
    finally:
        eng.close()


@pytest.mark.parametrize("wide,form", FORMS)
@pytest.mark.parametrize("option", [5, 6])
def test_chain_nowait_leaves_nothing_behind(F, cora, option, wide, form):
    """f2v_test_chain_nowait(1): an epoch whose launches wait for no row (rows are read early: its numbers are wrong and not looked
    at; it touches no memory a normal run does not).  Switched off again and started over, the handle gives a fresh handle's bits."""
    from force2vec_amd import _lib
    T = _lib.selftest_lib()
    X0, want = fresh(F, cora, option, wide, form)
    eng = engine(F, cora, wide)
    try:
        eng.set_embeddings(X0)
        eng.srand(1)
        _lib.check(T.f2v_test_chain_nowait(eng._h, 1), T)
        eng.train(option, 1, BATCH)
        assert eng.get_param("last_train_form") == form
        _lib.check(T.f2v_test_chain_nowait(eng._h, 0), T)
        eng.set_embeddings(X0)
        eng.srand(1)
        eng.train(option, EPOCHS, BATCH)
        assert eng.get_param("last_train_form") == form
        assert np.array_equal(eng.get_embeddings().view(np.uint32), want)
    finally:
        eng.close()
