"""The handle's own buffers: every device array, pinned array and event of f2v_engine.hip belongs to an owner type,
and the five arrays of the launch plans are one PlanArray each.

Host test (no GPU): the source itself -- one call site each of hipFree, hipHostFree and hipEventDestroy (the owners' release), no
allocation or event creation outside the owners' member functions, and an f2v_destroy that names no buffer.  -m gpu, the training-side
twin of tests/test_workspace.py: ONE handle runs a sequence of f2v_train calls in which every buffer grows after it has been used and is
used again after the plans were dropped; after every call its matrix must equal, bit for bit, that of a fresh handle given the matrix
as it stood before the call, the same seed and the same settings.  Two shorter cases switch the look-inside hooks and the push exchange
off and on again on one handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden_graph_path

gpu = pytest.mark.gpu
ENGINE_SOURCE = os.path.join(ROOT, "force2vec_amd", "csrc", "f2v_engine.hip")
OWNERS = ("DevBuf", "HostBuf", "DevEvents", "DevTimer", "PlanArray")


def block(source, head):
    """-> the text from `head` to the brace that closes the first `{` behind it"""
    at = source.index(head)
    depth = 0
    for k in range(source.index("{", at), len(source)):
        depth += {"{": 1, "}": -1}.get(source[k], 0)
        if depth == 0:
            return source[at:k + 1]
    raise AssertionError("unbalanced braces behind " + head)


@pytest.fixture(scope="module")
def source():
    return open(ENGINE_SOURCE).read()


@pytest.fixture(scope="module")
def owners(source):
    """owner type -> its definition; every member function that allocates or frees is defined inside it"""
    return {name: block(source, "struct %s {" % name) for name in OWNERS}


@pytest.mark.parametrize("call,owner", [("hipFree(", "DevBuf"), ("hipHostFree(", "HostBuf"), ("hipEventDestroy(", "DevEvents")])
def test_every_free_is_the_owners_release(source, owners, call, owner):
    assert source.count(call) == 1
    assert call in block(owners[owner], "void release()")


@pytest.mark.parametrize("call", [r"\bhipMalloc\(", r"\bhipExtMallocWithFlags\(", r"\bhipHostMalloc\(", r"\bhipEventCreate"])
def test_allocations_and_events_are_made_by_the_owners_alone(source, owners, call):
    inside = sum(len(re.findall(call, text)) for text in owners.values())
    assert inside >= 1 and len(re.findall(call, source)) == inside


def test_destroy_lists_no_buffer(source):
    body = block(source, "int f2v_destroy(f2v_handle c)")
    assert not re.findall(r"\bd_\w+", body) and "hipFree" not in body and "hipEventDestroy" not in body
    order = [body.index(step) for step in ("hipSetDevice(c->device)", "push_detach(c)", "delete c", "hipStreamDestroy(stream)")]
    assert order == sorted(order)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
SCALE, D, NS = 15, 32, 5  # D = 32: rows of one 128-byte line, the narrowest that the HBM chained form takes
PLAIN, CHAIN, WIDE = 0, 1, 2  # "last_train_form"
# (what it is about, settings made before it, option, epochs, batch, the form meant, the most epochs one launch carries)
STEPS = [
    ("plain", {}, 5, 1, 8192, PLAIN, 1),                                  # items, tree nodes, partial sums and their flags
    ("wide", {}, 5, 1, 1024, WIDE, 1),                                    # workgroup programs and jobs ...
    ("wide, smaller", {}, 5, 1, 256, WIDE, 1),                            # ... and four times as many of them
    ("chain", {"chain_wide": 0}, 5, 1, 4096, CHAIN, 1),                   # the HBM chained form: workgroup descriptors
    ("chain, smaller", {}, 5, 1, 512, CHAIN, 1),
    ("plain, small pieces", {"hub_chunk": 4}, 5, 1, 8192, PLAIN, 1),      # many more pieces, tree nodes and partial-sum slots
    # hub_chunk 8: the longest row (5906 neighbours) then stays within fanin^2 = 1024 pieces -- no tree-node workgroups, which a launch
    # that carries several epochs cannot have
    ("ring", {"chain_wide": 1, "hub_chunk": 8}, 5, 3, 256, WIDE, 3),      # epochs chained in one launch: the ring is allocated ...
    ("ring, outgrown", {}, 5, 8, 256, WIDE, 8),                           # ... and outgrown
    ("walks", {}, 7, 2, 256, WIDE, 1),                                    # both walk buffers, the pinned slots, the sample ids
    ("walks again", {}, 7, 2, 256, WIDE, 1),
    ("plain again", {}, 5, 1, 8192, PLAIN, 1),
]
GROWS = [("wide, smaller", "wide"), ("chain, smaller", "chain"), ("plain, small pieces", "plain")]  # (the larger step, the smaller one)


def bits(eng):
    return eng.get_embeddings().view(np.uint32)


@gpu
def test_one_handle_through_growth_and_reuse_equals_fresh_handles_bit_for_bit():
    import force2vec_amd as F
    from force2vec_amd.graph import rmat_csr
    rowptr, colids = rmat_csr(SCALE, 16, seed=7)

    def run(eng, k, option, iters, batch, form, epochs):
        eng.srand(100 + k)
        eng.train(option, iters, batch, NS)
        got = (eng.get_param("last_train_form"), eng.get_param("last_wide_epochs"))
        print("step %d: form %d, epochs per launch %d, plan_resident_bytes %d" % ((k,) + got + (eng.get_param("plan_resident_bytes"),)))
        assert got == (form, epochs), (k, got)

    eng = F.Engine(rowptr, colids, D)
    settings, resident = {}, {}
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        for k, (name, params, option, iters, batch, form, epochs) in enumerate(STEPS):
            before = eng.get_embeddings()
            settings.update(params)
            for key, value in params.items():
                eng.set_param(key, value)
            run(eng, k, option, iters, batch, form, epochs)
            resident[name] = eng.get_param("plan_resident_bytes")
            fresh = F.Engine(rowptr, colids, D)
            try:
                for key, value in settings.items():
                    fresh.set_param(key, value)
                fresh.set_embeddings(before)
                run(fresh, k, option, iters, batch, form, epochs)
                assert np.array_equal(bits(eng), bits(fresh)), (k, name)
            finally:
                fresh.close()
        for larger, smaller in GROWS:
            assert resident[larger] > 1.5 * resident[smaller], (larger, resident[larger], smaller, resident[smaller])
    finally:
        eng.close()


DIM, BATCH, CHUNK, EPOCHS = 128, 256, 4, 2


def cora_engine(F, **params):
    rowptr, colids = F.read_mtx(golden_graph_path("cora.mtx"))
    eng = F.Engine(rowptr, colids, DIM, selftest=True)
    for key, value in dict({"hub_chunk": CHUNK}, **params).items():
        eng.set_param(key, value)
    return eng


def start_and_result(F, train, **params):
    """-> (start, result as uint32) of a fresh handle that runs `train` once, without any hook or exchange"""
    eng = cora_engine(F, **params)
    try:
        eng.srand(1)
        eng.init_embeddings(0)
        X0 = eng.get_embeddings()
        eng.srand(1)
        train(eng)
        return X0, bits(eng)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("hook,params,form", [("f2v_test_stamps", {}, WIDE), ("f2v_test_xcd_times", {"chain_batches": 0}, PLAIN)])
def test_a_hook_switched_on_off_and_on_again_changes_no_bit(hook, params, form):
    """f2v_test_stamps (4 words per row, chained launches) and f2v_test_xcd_times (32 words, one launch per minibatch): the buffer is
    allocated, freed and allocated again on one handle, with a training call after every switch; the second buffer is filled like the
    first."""
    import force2vec_amd as F
    from force2vec_amd import _lib
    T = _lib.selftest_lib()
    X0, want = start_and_result(F, lambda e: e.train(5, EPOCHS, BATCH), **params)
    eng = cora_engine(F, **params)
    words = 4 * eng.n if hook == "f2v_test_stamps" else 32
    try:
        seen = []
        for on in (1, 0, 1):
            out = np.zeros(words, dtype=np.uint64)
            _lib.check(getattr(T, hook)(eng._h, on, None), T)
            eng.set_embeddings(X0)
            eng.srand(1)
            eng.train(5, EPOCHS, BATCH)
            assert eng.get_param("last_train_form") == form
            assert np.array_equal(bits(eng), want), (hook, on)
            if on:
                _lib.check(getattr(T, hook)(eng._h, 1, out.ctypes.data_as(C.POINTER(C.c_uint64))), T)
                seen.append(out)
        filled = [(s.reshape(-1, 4)[:, 2] != 0) if hook == "f2v_test_stamps" else (s[24:] != 0) for s in seen]  # rows stored | workgroups counted per XCD
        assert filled[0].all() and filled[1].all()
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize("landing", [0, 1])
def test_export_attach_detach_and_again_on_one_handle(landing):
    """f2v_push_export allocates fresh flags (and, in landing-buffer mode, a fresh landing buffer) for every attachment: export, attach
    (f2v_test_push_attach_local, this handle its own and only peer: one card), a sharded epoch, detach -- twice; the second epoch equals
    the first, which equals f2v_train's."""
    import force2vec_amd as F
    from force2vec_amd import _lib
    T = _lib.selftest_lib()
    X0, want = start_and_result(F, lambda e: e.train(5, 1, 1024))
    eng = cora_engine(F, push_landing=landing)
    try:
        for attachment in range(2):
            eng.set_embeddings(X0)
            eng.srand(1)
            eng.push_export()
            _lib.check(T.f2v_test_push_attach_local(eng._h, 0, 1, (C.c_void_p * 1)(eng._h)), T)
            eng.push_selftest()
            eng.train_sharded(5, 1, 1024)
            assert np.array_equal(bits(eng), want), attachment
            eng.push_detach()
    finally:
        eng.close()
