"""The greedy matrix's cases reach what greedy_matrix.py claims for them -- pinned on the oracle alone
(OracleGreedy.record() and the oracle env), over the same full-batch drive the GPU test runs, so a
case whose seed, T or shape stops reaching its edge fails here, without a GPU."""
import numpy as np
import pytest

import greedy_matrix as M
import oracle as O

MV = O.MOVE_CODES
# the move codes a map allows: a 1-row map has no U / D neighbour in bounds, a 1-column map no L / R
ALLOWED = {"ROW": {MV["S"], MV["L"], MV["R"]}, "COL": {MV["S"], MV["U"], MV["D"]}}


@pytest.fixture(scope="module")
def probes():
    out = {}
    for c in M.CASES:
        p = M.Probe(c)
        p.far_wanted = c.id == "SERP"
        M.run_full(M.OracleSide(c, probe=p), 2 * c.T + 3)
        out[c.id] = p
    return out


def test_case_limits():
    assert [c.id for c in M.CASES] == ["P1", "PK", "P64", "P65", "P128", "P129", "A19", "A20", "A64", "ROOMS",
                                       "ROOMS65", "ROW", "COL", "SERP", "MIX"]
    for c in M.CASES:
        assert c.E <= 16 and c.T <= 80
    mix = M.BY_ID["MIX"]
    shapes = [g.shape for g in M.case_grids(mix)]
    assert mix.maps[0] == M.S64 and shapes[0] == (64, 64) and len(set(shapes)) >= 3
    assert all(g.size <= shapes[0][0] * shapes[0][1] for g in M.case_grids(mix))   # table 0 is the largest
    em = M.case_env_map(mix)
    assert sorted(set(em)) == [0, 1, 2, 3] and (np.diff(em) >= 0).all()            # contiguous groups, in order


def test_synthetic_maps():
    rooms = M.rooms_grid()
    assert rooms.shape == (9, 13) and len(set(M.components(rooms)[rooms == 0])) == 2
    serp = M.serpentine_grid()
    assert serp.shape == (64, 64) and len(set(M.components(serp)[serp == 0])) == 1
    d = M.bfs_from(serp, (1, 0))
    assert d.max() == (serp == 0).sum() - 1 == 2078                 # one path through every free cell
    assert d.max() < 0xffff                                         # and it fits the tables' u16
    assert M.SYNTHETIC["row"]().shape == (1, 12) and M.SYNTHETIC["col"]().shape == (9, 1)


@pytest.mark.parametrize("cid", [c.id for c in M.CASES])
def test_moves_ops_deliveries(probes, cid):
    p = probes[cid]
    assert p.moves == ALLOWED.get(cid, set(MV.values())), f"move codes emitted: {sorted(p.moves)}"
    assert p.ops == {0, 1, 2}
    if cid != "SERP":
        assert p.deliveries.sum() >= 1
    assert p.overflow == 0, "n <= P + k everywhere, so the device's flags must stay 0"
    c = M.BY_ID[cid]
    assert p.max_n == (2 * c.P if c.P <= M.spawn_k(c.A) else c.P + M.spawn_k(c.A))
    if c.P > M.spawn_k(c.A):
        assert p.shifted >= 1, "no robot-step with list[target - 1] != target"
        # list[id - 1] = id for id <= k and id - k past it: no target names a package record past
        # max(k, P - k) - 1 (54 in P64, not 63)
        assert 0 <= p.tj_max <= max(M.spawn_k(c.A), c.P - M.spawn_k(c.A)) - 1


def test_list_lengths(probes):
    assert probes["P1"].max_n == 2 and probes["PK"].max_n == 10
    assert probes["P64"].max_n == 73 > 64
    assert probes["P129"].max_n == 150 > 128
    assert probes["A19"].max_n == 80 and probes["A20"].max_n == 81      # k = 20 | 21


@pytest.mark.parametrize("cid,index", [("P64", 64), ("P128", 64), ("P129", 128), ("A64", 128)])
def test_choices_past_the_first_scan_trips(probes, cid, index):
    """A long list alone does not need the later trips of the closest-free scan: a choice has to take
    an entry there (second trip: index >= 64, third: >= 128)."""
    assert probes[cid].pick_max >= index


@pytest.mark.parametrize("cid", ["P128", "P129", "A64"])
def test_targets_past_lane_63(probes, cid):
    assert probes[cid].tj_ge64 >= 1


@pytest.mark.parametrize("cid", ["P64", "P65"])
def test_targets_up_to_lane_63(probes, cid):
    """P64 and P65 cannot name a package record >= 64 (that takes P >= 65 + k): P65 is on the
    global-load path with every index still below 64."""
    assert probes[cid].tj_ge64 == 0


@pytest.mark.parametrize("cid", ["P65", "P128", "P129", "A64", "ROOMS65"])
def test_spawns_past_id_64(probes, cid):
    assert probes[cid].spawn_gt64 >= 1


@pytest.mark.parametrize("cid", ["ROOMS", "ROOMS65"])
def test_unreachable_goals(probes, cid):
    assert probes[cid].other_comp >= 1


def test_connected_maps_have_no_unreachable_goal(probes):
    for cid, p in probes.items():
        if not cid.startswith("ROOMS"):
            assert p.other_comp == 0, cid


def test_closest_free_choices(probes):
    assert any(p.tie for p in probes.values()), "no choice between tied entries of different packages"
    assert any(p.not_lowest for p in probes.values()), "every choice took the lowest free index"


def test_serpentine_depth(probes):
    assert probes["SERP"].far >= 1


def test_mix_every_group_delivers(probes):
    assert (probes["MIX"].deliveries >= 1).all(), probes["MIX"].deliveries


def test_record_layout():
    """The decoder's layout for the shapes of the matrix: list 4-aligned behind the two i16 arrays,
    free right behind the list, stride a multiple of 16 that holds them."""
    for c in M.CASES:
        L = M.record_layout(c.A, c.P)
        assert L["cap"] == 3 * c.P + 64 and L["list_off"] % 4 == 0 and 0 <= L["list_off"] - (8 + 4 * c.A) < 4
        assert L["free_off"] == L["list_off"] + 2 * L["cap"]
        assert L["stride"] % 16 == 0 and 0 <= L["stride"] - (L["free_off"] + L["cap"]) < 16
    row = np.zeros(M.record_layout(3, 2)["stride"], np.uint8)
    row[:8].view(np.int32)[:] = (2, 0)
    row[8:20].view(np.int16)[:] = (1, 0, 2, 0, 5, 0)
    row[20:24].view(np.uint16)[:] = (1, 2)
    row[20 + 2 * 70:20 + 2 * 70 + 2] = (1, 0)
    rec = M.decode_record(row, 3, 2)
    assert rec["n"] == 2 and rec["target"].tolist() == [1, 0, 2] and rec["prev_carry"].tolist() == [0, 5, 0]
    assert rec["list"].tolist() == [1, 2] and rec["free"].tolist() == [1, 0]
