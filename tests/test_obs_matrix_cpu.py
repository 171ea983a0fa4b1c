"""tests/obs_matrix.py without a GPU: every case's symbol and path facts follow from the selection rule
as obs_ref.py restates it, the tabled pairs really straddle their edges, the table reaches all 18
builder symbols and every path fact in both tracker modes, and every case's input conditions hold on
the oracle's trace (test_gpu_obs_matrix.py asserts the same before it runs the engine)."""
import pytest

import obs_matrix as M
import obs_ref as R
import oracle as O

FACTS = ("small", "RL", "sw", "one_pass", "gen_sort", "gen_map")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    O.build()


def _shapes(case):
    return [g.shape for g in R.grids(case)]


def _max_hw(case):
    return max(H * W for H, W in _shapes(case))


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_case_follows_from_the_rule(case):
    f = R.select(case)
    assert case.symbol == f["symbol"] and case.symbol in M.SYMBOLS
    assert {k: getattr(case, k) for k in FACTS} == {k: f[k] for k in FACTS}
    for g in R.grids(case):
        assert int((g == 0).sum()) >= max(case.A, 2), "the map has room for the robots"
    assert 9 <= case.E <= 13 and case.E % 4, "a launch of 4-wave workgroups has a last partial one"
    assert case.T == 25 or case.id[0] == "K"
    assert M.n_steps(case) == (2 * case.T + 3 if case.steps is None else case.steps)
    if case.env_map is not None:
        assert len(case.env_map) == case.E
        assert [n for _, n, _ in R.groups(case)] == ([5, 6] if case.id == "M1s" else [3, 4, 4])


def test_edge_pairs_straddle_their_edges():
    q = {
        "tuple_lanes": lambda c: R.tuple_lanes(c.A, c.P, c.MP),
        "rank_table_bytes": lambda c: max(R.rank_table_bytes(H, W) for H, W in _shapes(c)),
        "small_lds": lambda c: R.obs_small_lds(c.A, _max_hw(c), c.P, c.MO, c.MP),
        "key7_T": lambda c: c.T,
        "key32_T": lambda c: c.T,
        "plane_words": lambda c: R.plane_words(c.A, _max_hw(c)),
    }
    limit = dict(tuple_lanes=64, rank_table_bytes=8192, small_lds=16384, plane_words=2048)
    for what, lo, vlo, hi, vhi in M.EDGES:
        a, b = M.BY_ID[lo], M.BY_ID[hi]
        assert (q[what](a), q[what](b)) == (vlo, vhi), what
        if what in limit:
            assert vlo <= limit[what] < vhi, what
    # the two sides differ in nothing but the quantity's own parameter, and take the two paths
    a, b = M.BY_ID["S2a"], M.BY_ID["S2b"]
    assert a._replace(id="", MP=0, E=0, tracker="", symbol="", RL=None, one_pass=None) == \
        b._replace(id="", MP=0, E=0, tracker="", symbol="", RL=None, one_pass=None)
    assert (a.one_pass, b.one_pass, a.RL, b.RL) == (True, False, False, True)
    a, b = M.BY_ID["S10b"], M.BY_ID["S10a"]
    assert (a.RL, b.RL, a.one_pass, b.one_pass) == (True, False, False, False)
    assert (a.A, a.P, a.MO, a.MP, a.MR, a.MPs) == (b.A, b.P, b.MO, b.MP, b.MR, b.MPs)
    assert _shapes(a) == [(32, 32)] and _shapes(b) == [(33, 33)]
    a, b = M.BY_ID["S11a"], M.BY_ID["S11b"]
    assert (a.small, b.small, b.P - a.P) == (True, False, 1)
    c, d = M.BY_ID["S11c"], M.BY_ID["S11d"]
    assert R.obs_small_lds(c.A, 400, c.P, c.MO, c.MP) == 16256 and c.RL is False   # table + 4 slices > 64 KiB
    assert R.rank_table_bytes(20, 20) + 4 * 16256 > 65536 >= R.rank_table_bytes(20, 20) + 4 * 14960
    assert R.obs_small_lds(d.A, 400, d.P, d.MO, d.MP) == 14960 and d.RL is True
    # the key budgets: the T pairs are neighbours, and the budget flips between them and nowhere else
    for lo, hi, idx in (("K7a", "K7b", 0), ("K32a", "K32b", 1)):
        a, b = M.BY_ID[lo], M.BY_ID[hi]
        assert b.T == a.T + 1 and a._replace(T=0, obsT=0, steps=0, id="", tracker="", symbol="", E=0, small=None,
                                             RL=None, sw=None, one_pass=None, gen_sort=None, gen_map=None)[1:4] == \
            (b.maps, b.A, b.P)
        ka, kb = R.key_budgets(_shapes(a), a.T), R.key_budgets(_shapes(b), b.T)
        assert ka[idx] > 0 and kb[idx] == 0
    assert (M.BY_ID["K7a"].small, M.BY_ID["K7b"].small) == (True, False)
    assert (M.BY_ID["K7b"].gen_sort, M.BY_ID["K32a"].gen_sort, M.BY_ID["K32b"].gen_sort) == ("slow", "fast", "slow")
    assert R.obs_small_lds(3, 4096, 64, 2, 20) == 15056 and R.obs_small_lds(4, 4096, 64, 3, 5) == 18128
    assert R.plane_words(2, 4096) == 2048 and M.BY_ID["S9bg"].gen_map == ("planes",)
    a, b = M.BY_ID["G3a"], M.BY_ID["G3b"]
    assert (a.gen_map, b.gen_map, b.A - a.A) == (("planes",), ("bitrows",), 1)


def test_table_reaches_every_symbol_and_fact_in_both_tracker_modes():
    assert len(M.SYMBOLS) == len(set(M.SYMBOLS)) == 18
    reached = set()
    for c in M.CASES:
        reached |= {c.symbol, R.half_symbol(c.symbol, "float16"), R.half_symbol(c.symbol, "bfloat16")}
    assert reached == set(M.SYMBOLS)
    seen = {}
    for c in M.CASES:
        for k in FACTS:
            v = getattr(c, k)
            for x in (v if isinstance(v, tuple) else (v,)):
                if x is not None:
                    seen.setdefault((k, x), set()).add(c.tracker)
    want = {(k, v) for k in ("small", "RL", "sw", "one_pass") for v in (True, False)}
    want |= {("gen_sort", "fast"), ("gen_sort", "slow"), ("gen_map", "planes"), ("gen_map", "bitrows"),
             ("gen_map", "elem")}
    assert set(seen) == want
    assert all(m == {"mappo", "fresh"} for m in seen.values()), {k: m for k, m in seen.items() if len(m) < 2}
    # the three package-order paths of the small builder are chosen per env by want: named cases reach them
    assert {c.A for c in M.CASES if c.small} >= {1, 2, 3, 4, 5, 6, 7, 8}
    # the masked test: the one-launch kernel (single map and per-env maps) and the general builder's mask
    assert [(M.BY_ID[i].small, M.BY_ID[i].env_map is not None) for i in M.MASKED] == \
        [(True, False), (True, False), (False, False), (True, True)]
    assert len({g.shape for g in R.grids(M.BY_ID["M1s"])}) == 1 < len({g.shape for g in R.grids(M.BY_ID["M1"])})


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_input_conditions_hold_on_the_oracle_trace(case):
    R.check_inputs(case)


def test_want_reaches_zero_and_the_recorded_package_ties():
    c4, c6 = R.conditions(M.BY_ID["S4"]), R.conditions(M.BY_ID["S6"])
    assert 0 in (c4["want"] | c6["want"]), "S4 plus S6: no compared row with want = 0"
    # want on both sides of 6 | 7 with A == 5 (the interleaved bitonic networks) and A != 5 (sort64 per agent)
    for cid in ("S4", "S4m", "S5"):
        w = R.conditions(M.BY_ID[cid])["want"]
        assert min(w) <= 6 < max(w), (cid, sorted(w))
    no_tie = tuple(c.id for c in M.CASES if R.conditions(c)["pkg_tie"] == 0)
    assert no_tie == M.NO_PKG_TIE
