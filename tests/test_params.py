"""The parameter interface (include/f2v.h: f2v_set_param / f2v_get_param), name by name: which names can be set, which can be read,
the accepted values, the error code and text of a rejected value, that a rejected value leaves the stored one alone, and which names
drop the launch plans when they are set ("plan_resident_bytes" goes to 0): always, only when the value changes, or never.

Everything here is host-side validation and value round trips on the karate graph; the only device work is a one-epoch f2v_train
that makes launch plans to drop."""
import ctypes as C

import pytest

from conftest import golden_graph_path

import force2vec_amd as F
from force2vec_amd import _lib

pytestmark = pytest.mark.gpu

DIM, BATCH = 64, 16
ALWAYS, ON_CHANGE, NEVER = "always", "on change", "never"

# name: (values that are accepted, [(rejected value, error text)], replan rule); a name of GET_ONLY / SET_ONLY aside, every name reads back
SETTABLE = {
    "hub_chunk": ([16, 0, 8], [(-1, "hub_chunk out of range"), (0x80000000, "hub_chunk out of range"), (1 << 28, "hub_chunk out of range")], ALWAYS),
    "hub_chunk_for_batch": ([BATCH, 0xFFFFFFFF], [(0, "hub_chunk_for_batch: bad batch size"), (-1, "hub_chunk_for_batch: bad batch size"),
                                                  (1 << 32, "hub_chunk_for_batch: bad batch size")], ON_CHANGE),
    "hub_fanin": ([8, 0, 2, 32], [(1, "hub_fanin must be 0 (one sequential pass) or >= 2"), (-1, "hub_fanin must be 0 (one sequential pass) or >= 2"),
                                  (0x80000000, "hub_fanin must be 0 (one sequential pass) or >= 2")], ALWAYS),
    "quarter_wave": ([0, 1], [], ON_CHANGE),
    "fast_rng": ([1, 0], [], NEVER),
    "use_graph": ([1, 0], [], NEVER),
    "class_cut": ([0, 1], [], ALWAYS),
    "piece_affinity": ([0, 1], [], ON_CHANGE),
    "count_compulsory": ([1, 0], [], ON_CHANGE),
    "rows_in_flight": ([4, 8, 0], [(5, "rows_in_flight must be 0 (default), 4 or 8"), (-4, "rows_in_flight must be 0 (default), 4 or 8")], NEVER),
    "push_fused": ([0, 1], [], NEVER),
    "merge_finalize": ([0, 1], [], NEVER),
    "chain_batches": ([0, 1], [], NEVER),
    "chain_max_batch": ([0, 0xFFFFFFFF, 4096], [(-1, "chain_max_batch out of range"), (1 << 32, "chain_max_batch out of range")], NEVER),
    "wide_epochs": ([1024, 1, 0], [(-1, "wide_epochs must be 0 (automatic) ... 1024"), (1025, "wide_epochs must be 0 (automatic) ... 1024")], NEVER),
    "wide_single": ([1, 0], [], NEVER),
    "replicate_small": ([0, 2, 1], [(-1, "replicate_small must be 0 (never), 1 (where no peer shares the GPU) or 2 (always)"),
                                    (3, "replicate_small must be 0 (never), 1 (where no peer shares the GPU) or 2 (always)")], NEVER),
    "wide_samples_early": ([0, 1, -1], [(-2, "wide_samples_early must be -1 (automatic), 0 or 1"), (2, "wide_samples_early must be -1 (automatic), 0 or 1")], NEVER),
    "wide_min_width": ([16, 32, 64, 128, 0], [(48, "wide_min_width must be 0 (automatic), 16, 32, 64 or 128"), (256, "wide_min_width must be 0 (automatic), 16, 32, 64 or 128"),
                                              (-16, "wide_min_width must be 0 (automatic), 16, 32, 64 or 128")], ALWAYS),
    "wide_max_batch": ([0, 0xFFFFFFFF, 2048], [(-1, "wide_max_batch out of range"), (1 << 32, "wide_max_batch out of range")], NEVER),
    "wide_rows": ([2, 0x7FFFFFFF, 262144], [(1, "wide_rows out of range"), (0x80000000, "wide_rows out of range")], ALWAYS),
    "chain_rows": ([2, 0x7FFFFFFF, 65536], [(1, "chain_rows out of range"), (0x80000000, "chain_rows out of range")], ALWAYS),
    "tree_timeout_ms": ([1, 600000, 5000], [(0, "tree_timeout_ms must be 1..600000"), (600001, "tree_timeout_ms must be 1..600000")], NEVER),
    "epoch_marks": ([3, 0x7FFFFFFF, 0], [(-1, "epoch_marks out of range"), (0x80000000, "epoch_marks out of range")], NEVER),
    "chain_wide": ([0, 1], [], ALWAYS),
    "wide_phases": ([64, 1], [(0, "wide_phases must be 1..64"), (65, "wide_phases must be 1..64")], ALWAYS),
    "wide_span": ([1, 64, 2], [(0, "wide_span must be 1..64"), (65, "wide_span must be 1..64")], ALWAYS),
    "wide_finish": ([1, 64, 4], [(0, "wide_finish must be 1..64"), (65, "wide_finish must be 1..64")], ALWAYS),
    "wide_order": ([1, 2, 0], [(-1, "wide_order must be 0, 1 or 2"), (3, "wide_order must be 0, 1 or 2")], ALWAYS),
    "wide_rounds": ([1, 64, 0], [(-1, "wide_rounds must be 0..64"), (65, "wide_rounds must be 0..64")], ALWAYS),
    "loss_every": ([2, 0x7FFFFFFF, 0], [(-1, "loss_every out of range"), (0x80000000, "loss_every out of range")], NEVER),
    "loss_seed": ([7, -1, 1], [], NEVER),
    "nearest_splits": ([256, 1, 0], [(-1, "nearest_splits must be 0..256"), (257, "nearest_splits must be 0..256")], NEVER),
    "nearest_block": ([32, 128, 0], [(64, "nearest_block must be 0, 32 or 128"), (-32, "nearest_block must be 0, 32 or 128")], NEVER),
    "nearest_chunk": ([1, 65536, 8192], [(0, "nearest_chunk must be 1..65536"), (65537, "nearest_chunk must be 1..65536")], NEVER),
    "chain_timeout_ms": ([1, 600000, 200], [(0, "chain_timeout_ms must be 1..600000"), (600001, "chain_timeout_ms must be 1..600000")], NEVER),
    "recover": ([0, 1], [], NEVER),
    "push_landing": ([1, 0], [], NEVER),
    "push_timeout_ms": ([1, 600000, 20000], [(0, "push_timeout_ms must be 1..600000"), (600001, "push_timeout_ms must be 1..600000")], NEVER),
    "waves_per_block": ([1, 2, 4], [(0, "waves_per_block must be 1, 2 or 4"), (3, "waves_per_block must be 1, 2 or 4"), (8, "waves_per_block must be 1, 2 or 4")], ON_CHANGE),
}
BOOLEANS = [name for name, (_, bad, _) in SETTABLE.items() if not bad and name != "loss_seed"]
SET_ONLY = ["rows_in_flight", "hub_chunk_for_batch"]
GET_ONLY = ["shared_card", "hub_chunk_auto", "last_loss_us", "last_train_replicated", "plan_resident_bytes", "last_wide_epochs", "last_train_form",
            "last_wide_width", "last_wide_early", "recoveries", "xcc_count", "xcc_round_robin", "push_world", "push_rank", "dim", "n", "nnz"]


class Handle:
    """One engine on the karate graph, driven through the C entry points so that codes and messages are seen as they are."""

    def __init__(self, dim=DIM):
        rowptr, colids = F.read_mtx(golden_graph_path("karate.mtx"))
        self.engine = F.Engine(rowptr, colids, dim)
        self.L, self.h = self.engine._L, self.engine._h

    def set(self, name, value):
        rc = self.L.f2v_set_param(self.h, name.encode(), value)
        return rc, self.L.f2v_last_error().decode() if rc != _lib.F2V_OK else ""

    def get(self, name):
        v = C.c_int64(-12345)
        rc = self.L.f2v_get_param(self.h, name.encode(), C.byref(v))
        return rc, (self.L.f2v_last_error().decode() if rc != _lib.F2V_OK else ""), v.value

    def value(self, name):
        rc, msg, v = self.get(name)
        assert rc == _lib.F2V_OK, (name, msg)
        return v

    def train(self):
        self.engine.srand(1)
        self.engine.init_embeddings(_lib.INIT_SYMMETRIC)
        self.engine.train(5, 1, BATCH)
        assert self.value("plan_resident_bytes") > 0


@pytest.fixture()
def h():
    handle = Handle()
    yield handle
    handle.engine.close()


def test_tables_name_every_parameter_once():
    assert not set(SET_ONLY) - set(SETTABLE) and not set(GET_ONLY) & set(SETTABLE)
    assert len(SETTABLE) == 40 and len(GET_ONLY) == 17


@pytest.mark.parametrize("name", sorted(SETTABLE))
def test_accepted_values_read_back(h, name):
    good, _, _ = SETTABLE[name]
    for v in good:
        assert h.set(name, v) == (_lib.F2V_OK, ""), (name, v)
        if name == "hub_chunk_for_batch":  # resolves the automatic chunk: 4 for any minibatch of this graph
            assert (h.value("hub_chunk"), h.value("hub_chunk_auto")) == (4, 1)
        elif name in SET_ONLY:
            rc, msg, _ = h.get(name)
            assert (rc, msg) == (_lib.F2V_EINVAL, "f2v_get_param: unknown parameter '%s'" % name)
        else:
            assert h.value(name) == v, (name, v)
        if name == "hub_chunk":
            assert h.value("hub_chunk_auto") == 0
        if name == "chain_rows":  # an explicit value holds for both chained forms
            assert h.value("wide_rows") == v
        if name == "wide_rows":
            assert h.value("chain_rows") == 65536


@pytest.mark.parametrize("name", BOOLEANS)
def test_booleans_take_any_nonzero_value_as_true(h, name):
    for v, want in ((7, 1), (0, 0), (-1, 1), (1 << 40, 1)):
        assert h.set(name, v) == (_lib.F2V_OK, ""), (name, v)
        assert h.value(name) == want, (name, v)


@pytest.mark.parametrize("name", sorted(n for n in SETTABLE if SETTABLE[n][1]))
def test_rejected_values_change_nothing(h, name):
    good, bad, _ = SETTABLE[name]
    assert h.set(name, good[0])[0] == _lib.F2V_OK
    before = {n: h.value(n) for n in list(SETTABLE) + GET_ONLY if n not in SET_ONLY}
    for v, text in bad:
        assert h.set(name, v) == (_lib.F2V_EINVAL, text), (name, v)
        assert {n: h.value(n) for n in before} == before, (name, v)


def test_nearest_block_128_needs_a_dim_that_fits(h):
    wide = Handle(dim=256)
    try:
        assert wide.set("nearest_block", 32)[0] == _lib.F2V_OK
        assert wide.set("nearest_block", 128) == (_lib.F2V_EINVAL, "nearest_block = 128 needs dim <= 128 (the query block lives in LDS)")
        assert wide.value("nearest_block") == 32
        assert wide.set("nearest_block", 64) == (_lib.F2V_EINVAL, "nearest_block must be 0, 32 or 128")
    finally:
        wide.engine.close()
    assert h.set("nearest_block", 128)[0] == _lib.F2V_OK and h.value("nearest_block") == 128


@pytest.mark.parametrize("name", GET_ONLY)
def test_read_only_names(h, name):
    rc, msg, v = h.get(name)
    assert (rc, msg) == (_lib.F2V_OK, "") and v != -12345
    assert h.set(name, 1) == (_lib.F2V_EINVAL, "f2v_set_param: unknown parameter '%s'" % name)
    assert h.value(name) == v
    want = {"dim": DIM, "n": h.engine.n, "nnz": h.engine.nnz, "hub_chunk_auto": 1, "shared_card": 0, "push_world": 0, "push_rank": 0, "recoveries": 0,
            "plan_resident_bytes": 0, "last_wide_epochs": 1, "last_train_form": 0, "last_loss_us": 0, "last_train_replicated": 0}
    if name in want:
        assert v == want[name]


def test_unknown_name_and_null_arguments(h):
    assert h.set("no_such_parameter", 1) == (_lib.F2V_EINVAL, "f2v_set_param: unknown parameter 'no_such_parameter'")
    rc, msg, v = h.get("no_such_parameter")
    assert (rc, msg, v) == (_lib.F2V_EINVAL, "f2v_get_param: unknown parameter 'no_such_parameter'", -12345)
    assert h.set("", 1) == (_lib.F2V_EINVAL, "f2v_set_param: unknown parameter ''")
    out = C.c_int64()
    assert h.L.f2v_set_param(None, b"hub_chunk", 1) == _lib.F2V_EINVAL and h.L.f2v_last_error() == b"f2v_set_param: null argument"
    assert h.L.f2v_set_param(h.h, None, 1) == _lib.F2V_EINVAL and h.L.f2v_last_error() == b"f2v_set_param: null argument"
    assert h.L.f2v_get_param(None, b"hub_chunk", C.byref(out)) == _lib.F2V_EINVAL and h.L.f2v_last_error() == b"f2v_get_param: null argument"
    assert h.L.f2v_get_param(h.h, None, C.byref(out)) == _lib.F2V_EINVAL and h.L.f2v_last_error() == b"f2v_get_param: null argument"
    assert h.L.f2v_get_param(h.h, b"hub_chunk", None) == _lib.F2V_EINVAL and h.L.f2v_last_error() == b"f2v_get_param: null argument"


def test_defaults(h):
    want = {"hub_chunk": 64, "hub_fanin": 32, "quarter_wave": 1, "fast_rng": 0, "use_graph": 0, "class_cut": 1, "piece_affinity": 1, "count_compulsory": 0,
            "push_fused": 1, "chain_batches": 1, "chain_max_batch": 4096, "wide_epochs": 0, "wide_single": 0, "replicate_small": 1, "wide_samples_early": -1,
            "wide_min_width": 0, "wide_max_batch": 2048, "wide_rows": 262144, "chain_rows": 65536, "epoch_marks": 0, "chain_wide": 1, "wide_phases": 1,
            "wide_span": 2, "wide_finish": 4, "wide_order": 0, "wide_rounds": 0, "loss_every": 0, "loss_seed": 1, "nearest_splits": 0, "nearest_block": 0,
            "nearest_chunk": 8192, "push_landing": 0, "push_timeout_ms": 20000, "waves_per_block": 4}
    assert {n: h.value(n) for n in want} == want


@pytest.mark.parametrize("name", sorted(n for n in SETTABLE if SETTABLE[n][2] == ALWAYS))
def test_setting_the_current_value_drops_the_plans(h, name):
    h.train()
    assert h.set(name, h.value(name))[0] == _lib.F2V_OK
    assert h.value("plan_resident_bytes") == 0


@pytest.mark.parametrize("name", sorted(n for n in SETTABLE if SETTABLE[n][2] == ON_CHANGE))
def test_only_a_new_value_drops_the_plans(h, name):
    h.train()
    if name == "hub_chunk_for_batch":  # the chunk this batch size resolves to is the one the f2v_train above ran with
        assert h.set(name, BATCH)[0] == _lib.F2V_OK
        assert h.value("plan_resident_bytes") > 0
        assert h.set("hub_chunk", 8)[0] == _lib.F2V_OK
        h.train()
        assert h.set(name, BATCH)[0] == _lib.F2V_OK  # back to 4
    else:
        current = h.value(name)
        assert h.set(name, current)[0] == _lib.F2V_OK
        assert h.value("plan_resident_bytes") > 0
        assert h.set(name, next(v for v in SETTABLE[name][0] if v != current))[0] == _lib.F2V_OK
    assert h.value("plan_resident_bytes") == 0


def test_other_names_keep_the_plans(h):
    h.train()
    resident = h.value("plan_resident_bytes")
    for name in sorted(n for n in SETTABLE if SETTABLE[n][2] == NEVER):
        for v in SETTABLE[name][0]:
            assert h.set(name, v)[0] == _lib.F2V_OK
        assert h.value("plan_resident_bytes") == resident, name
