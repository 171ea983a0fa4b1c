"""The collectors' shared graph bookkeeping (marl_gpu/_capture.py) on the CPU: which calls a
``GraphCache`` answers with a stored graph, the offset rule around a replay, and what ``eval_mode``
leaves behind.  A sentinel object stands in for the hipGraph; nothing here touches a GPU."""
import copy

import pytest

torch = pytest.importorskip("torch")

from marl_gpu._capture import GraphCache, Graphed, eval_mode, param_addresses  # noqa: E402


def linear():
    torch.manual_seed(0)
    return torch.nn.Linear(3, 2)


def test_param_addresses():
    m, t = linear(), torch.zeros(4)
    assert param_addresses(m) == (m.weight.data_ptr(), m.bias.data_ptr())
    assert param_addresses(m, t, "greedy", len) == (m.weight.data_ptr(), m.bias.data_ptr(), t.data_ptr())
    assert param_addresses("greedy", len) == ()


def test_same_module_hits_other_module_misses():
    m, G = linear(), object()
    c = GraphCache()
    assert c.lookup((m,), ()) is None and c.captured_graphs() == {} and not c.matches((m,), ())
    c.store((m,), (), None, G, 4)
    assert c.lookup((m,), ()) is G and c.lookup((m,), ()) is G
    assert c.captured_graphs() == {None: 4}
    twin = copy.deepcopy(m)                       # equal values, another object
    assert torch.equal(twin.weight, m.weight)
    assert c.lookup((twin,), ()) is None
    assert c.lookup((m, twin), ()) is None and c.lookup((), ()) is None


def test_load_state_dict_in_place_hits_rebound_data_misses():
    m, G = linear(), object()
    c = GraphCache()
    c.store((m,), (), None, G, 4)
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})   # copies into the same storage
    assert c.lookup((m,), ()) is G
    m.weight.data = m.weight.data.clone()                              # the parameter moved
    assert c.lookup((m,), ()) is None


def test_values_and_slots():
    m, G0, G1, G2 = linear(), object(), object(), object()
    c = GraphCache()
    c.store((m,), (5, True), 0, G0, 5)
    assert c.lookup((m,), (5, True), 0) is G0
    assert c.lookup((m,), (6, True), 0) is None and c.lookup((m,), (5, False), 0) is None
    assert c.lookup((m,), (5, True), 1) is None and c.lookup((m,), (5, True)) is None
    assert c.matches((m,), (5, True)) and not c.matches((m,), (6, True))
    c.store((m,), (5, True), 1, G1, 5)                                  # same key: both slots stay
    assert c.lookup((m,), (5, True), 0) is G0 and c.lookup((m,), (5, True), 1) is G1
    assert c.captured_graphs() == {0: 5, 1: 5} and len(c) == 2
    c.store((m,), (6, True), 1, G2, 6)                                  # a new key drops the old slots
    assert c.captured_graphs() == {1: 6}
    assert c.lookup((m,), (5, True), 0) is None and c.lookup((m,), (6, True), 1) is G2
    c.clear()
    assert c.captured_graphs() == {} and len(c) == 0 and c.lookup((m,), (6, True), 1) is None


def test_string_owner_by_value_tensor_owner_by_address():
    G = object()
    c = GraphCache()
    c.store(("greedy",), ("greedy", 8), "chunk", G, 8)
    assert c.lookup(("".join(["gre", "edy"]),), ("greedy", 8), "chunk") is G   # an equal string, not the same object
    assert c.lookup(("random",), ("greedy", 8), "chunk") is None
    tape = torch.zeros((4, 2, 2), dtype=torch.uint8)
    c.store((tape,), ("tape", 4), "chunk", G, 4)
    assert c.captured_graphs() == {"chunk": 4}
    assert c.lookup((tape,), ("tape", 4), "chunk") is G
    assert c.lookup((tape.clone(),), ("tape", 4), "chunk") is None
    tape.data = torch.ones((4, 2, 2), dtype=torch.uint8)                       # same object, other storage
    assert c.lookup((tape,), ("tape", 4), "chunk") is None


def test_cache_keeps_its_owners_alive():
    import gc
    import weakref
    m = linear()
    alive = weakref.ref(m)
    c = GraphCache()
    c.store((m,), (), None, object(), 1)
    del m
    gc.collect()
    assert alive() is not None     # so no new module can appear at the captured one's address
    c.clear()
    gc.collect()
    assert alive() is None


def test_replay_writes_the_host_offset_first_and_advances_it_after():
    class FakeGraph:   # what a captured region does to the counter: read the base, then mdl_counter_add
        def __init__(self, col, steps):
            self.col, self.steps, self.bases = col, steps, []

        def replay(self):
            self.bases.append(int(self.col._off_dev[0]))
            self.col._off_dev += self.steps

    col = Graphed()
    col._init_graphs("cpu")
    assert col.offset == 0 and col.captured_graphs() == {}
    chunk, rest = FakeGraph(col, 3), FakeGraph(col, 1)
    col._replay((chunk, chunk, rest), 7)
    assert chunk.bases == [0, 3] and rest.bases == [6] and col.offset == 7
    col.offset = 1000                       # an eager call, or a resumed run: the device copy is stale now
    col._replay((rest,), 1)
    assert rest.bases == [6, 1000] and col.offset == 1001
    col._graphs.store(("greedy",), (), "chunk", chunk, 3)
    assert col.captured_graphs() == {"chunk": 3}


def test_eval_mode_restores_training_modules_only():
    a, b = linear(), linear()
    b.eval()
    with eval_mode(a, b):
        assert not a.training and not b.training
    assert a.training and not b.training
    with pytest.raises(RuntimeError, match="boom"):
        with eval_mode(a, b):
            assert not a.training
            raise RuntimeError("boom")
    assert a.training and not b.training


def test_eval_mode_passes_plain_objects_through():
    a = linear()
    with eval_mode(len, "greedy", torch.zeros(2), a):
        assert not a.training
    assert a.training
    with eval_mode():
        pass
