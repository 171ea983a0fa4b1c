"""The inputs of tests/test_gpu_views_batch.py, from the generator and the oracle alone (tests/views_ref.py):
the conditions under which comparing the mdl_views_* entry points with the oracle means something.  An edit
of the generator that loses one of them fails here, on a machine without a GPU."""
import numpy as np

import views_ref as V

MDL_MAX_ROBOTS = 64


def _all():
    return V.batches().values()


def test_records_are_valid():
    """What include/mdl_engine.h asks of a view record: cells inside the view's map, a map index in range,
    n_slots <= max_slots, at most MDL_MAX_ROBOTS robots, status 1 or 2."""
    p = V.pool()
    for x in p.trans:
        H, W = V.maps()[x["map"]].shape
        assert 0 <= x["map"] < len(V.maps()) and 1 <= x["A"] <= MDL_MAX_ROBOTS and len(x["rows0"]) <= 40
        for rob in (x["rob0"], x["rob1"]):
            assert rob.shape == (x["A"], 3)
            assert (rob[:, 0] >= 0).all() and (rob[:, 0] < H).all() and (rob[:, 1] >= 0).all() and (rob[:, 1] < W).all()
        rows = x["rows0"]
        assert np.isin(rows[:, 1], (1, 2)).all()
        assert (rows[:, 2:6] >= 0).all() and (rows[:, [2, 4]] < H).all() and (rows[:, [3, 5]] < W).all()
        assert (x["mv"] < 5).all() and (x["op"] < 3).all()
    assert set(p.A) == set(V.ROBOTS)
    for b in _all():
        assert (b.ns <= b.max_slots).all() and b.max_slots == b.ns.max()


def test_blobs_are_packed_back_to_back():
    p = V.pool()
    for i, x in enumerate(p.trans):
        rec = p.prev[p.prev_off[i]:]
        assert rec[:4].tolist() == [x["t0"], x["A"], len(x["rows0"]), x["map"]]
        assert p.cur[p.cur_off[i]:p.cur_off[i] + 2].tolist() == [x["t1"], x["A"]]
    assert len(set(np.diff(p.prev_off))) > 10, "the record lengths vary"
    assert p.prev_off[-1] + 4 + 3 * p.A[-1] + 8 * p.ns[-1] == p.prev.size
    assert p.act_off[-1] + p.A[-1] == p.act.size
    unaligned = [b.name for b in _all() if (p.act_off[b.idx] % 4 != 0).any()]
    assert len(unaligned) >= len(V.batches()) - 3, "an action offset that is no multiple of 4, in nearly every batch"


def test_batch_shapes():
    names = set(V.batches())
    assert names == {f"{k}-{n}" for k in ("small", "large", "mixed") for n in (1, 5, 37)}
    assert set(V.FEATURE_BATCHES) | set(V.REWARD_BATCHES) <= names
    for b in _all():
        assert len(set(b.idx.tolist())) == b.n, "distinct records"
        if b.name in V.FEATURE_BATCHES:   # one map shape per features launch (include/mdl_engine.h)
            assert len({V.maps()[m].shape for m in b.map}) == 1, b.name
        if b.n >= 5:
            assert len(set(b.A)) >= 3 and len(set(b.ns)) >= 4, b.name
        assert (np.diff(b.op_off) > b.A[:-1]).all(), "a gap after every view's rewards"
    maps_seen = set(np.concatenate([b.map for b in _all()]).tolist())
    assert maps_seen == {0, 1, 2, 3}
    assert any({1, 2, 3} <= set(V.batches()[n].map.tolist()) for n in V.FEATURE_BATCHES), "maps 1, 2, 3 in one launch"
    assert any(len({V.maps()[m].shape for m in V.batches()[n].map}) == 2 for n in V.REWARD_BATCHES)


def test_slot_counts_reach_the_clamps():
    assert any((b.ns == 0).any() for b in _all()), "a view with n_slots == 0"
    hit = []
    for name in V.FEATURE_BATCHES:
        b = V.batches()[name]
        for MO, MP, MR, MPs in b.sizes():
            if b.max_slots >= MP and ((b.ns > 0) & (b.ns < MP)).any() and (b.ns > MP).any():
                hit.append((name, MP))
    assert len(hit) >= 4, f"0 < n_slots < MP <= max_slots next to n_slots > MP in one launch: {hit}"
    for b in _all():
        s = b.sizes()
        assert s[0] == V.TRUNCATING and s[1] == V.PADDING and s[1][1] > b.max_slots


def test_agent_indices():
    for b in _all():
        ok = (b.agent >= 0) & (b.agent < b.A)
        if b.n >= 5:
            assert (b.agent == -1).sum() == 1 and (b.agent == b.A).sum() == 1 and ok.sum() == b.n - 2, b.name
        else:
            assert ok.all()


def test_carrying_robots_and_transit_rows():
    p = V.pool()
    n = 0
    for b in _all():
        for i in b.idx:
            x = p.trans[i]
            held = set(x["rob0"][:, 2].tolist()) - {0}
            n += len(held & set(x["rows0"][x["rows0"][:, 1] == 2][:, 0].tolist()))
    assert n >= 20, "carrying robots whose package row is in transit"
    only = [x for b in _all() for x in (p.trans[i] for i in b.idx) if len(x["rows0"]) and (x["rows0"][:, 1] == 2).all()]
    assert only, "a record whose only slots are in transit"
    assert any(x["greedy"] for x in p.trans) and not all(x["greedy"] for x in p.trans)


def test_rewards_are_not_trivial():
    p = V.pool()
    for consts in V.CONSTS:
        sh = np.concatenate([V.shaped(n, consts) for n in V.REWARD_BATCHES])
        g = np.concatenate([p.g[V.batches()[n].idx] for n in V.REWARD_BATCHES]).astype(np.float32)
        assert (sh != g).mean() >= 0.25, consts
    assert (np.concatenate([V.shaped(n, "mappo") for n in V.REWARD_BATCHES]) !=
            np.concatenate([V.shaped(n, "qmix") for n in V.REWARD_BATCHES])).mean() >= 0.25
    ints = np.concatenate([r for n in V.REWARD_BATCHES for r in V.idq_reward(n, True)])
    strs = np.concatenate([r for n in V.REWARD_BATCHES for r in V.idq_reward(n, False)])
    assert (ints != 0).mean() >= 0.10
    assert (ints != strs).mean() >= 0.10, "the integer ops change the reward"


def test_features_differ_between_views():
    """The expected rows of a batch are all different (so a view read from another's offset, or written to
    another's row, shows), and map 3's views differ from what map 1's walls would give."""
    for name in V.FEATURE_BATCHES:
        b = V.batches()[name]
        f = V.features(name, b.sizes()[2])
        for k in ("obs", "vec", "gvec"):
            rows = {f[k][w].tobytes() for w in range(b.n)}
            assert len(rows) >= b.n - 2, (name, k, len(rows))   # the two out-of-range agents may coincide
        a = V.alt(name, V.alt_shapes(name)[1])
        assert len({a["qmix"][w].tobytes() for w in range(b.n)}) == b.n
    assert V.maps()[0].shape != V.maps()[1].shape == V.maps()[2].shape == V.maps()[3].shape
    assert not np.array_equal(V.maps()[3], V.maps()[1]) and not np.array_equal(V.maps()[3], V.maps()[2])
    for name in ("large-5", "large-37"):
        b = V.batches()[name]
        assert (b.map == 3).any() and (b.map != 3).any(), name
