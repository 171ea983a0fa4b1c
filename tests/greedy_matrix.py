"""The cases that run the batched greedy agent (csrc/mdl_greedy.hip: k_bfs_table, k_greedy_init,
k_greedy_act) against the oracle's agent (oracle.OracleGreedy, greedyagent.py restated) at the edges
of the kernel's shape decisions, the synthetic maps they need, the decoder of the agent record as a
checkpoint carries it, and the oracle-side driver.

What the kernel decides by shape (csrc/mdl_greedy.hip):
  P <= 64    the target package's record comes from its lane (ds_bpermute), else from a dependent
             global load pk[tj]; the spawns are appended in ceil(P / 64) chunks, the first from
             registers, the others from memory;
  nl         the closest-free scan takes ceil(nl / 64) trips over the list;
  A          robot lanes 0..A-1; the target choice reads lane i of every robot in turn;
  mi         tables + tab_off[mi] and the map's H, W select the BFS table of the env's map.
What the agent does whatever the shape (checked on the oracle alone by test_greedy_matrix_cpu.py):
  k = min(A, 20) + 1 packages spawn at t = 0 (all of them where P <= k) and are appended twice, by
  init_agents and by the first get_actions; ids follow the start-time sort, so list[id - 1] = id - k
  for id > k and the list never exceeds P + k entries (cap = 3P + 64 is never hit, flags stay 0).

This module only holds data and helpers; it is not a conftest."""
from __future__ import annotations

from collections import deque, namedtuple

import numpy as np

import oracle as O
from golden_io import grid

M1, M2, M3, S64 = "map1.txt", "map2.txt", "map3.txt", "synthetic64.txt"

# seed: env e is seeded seed + e.  env_map None: one map.  E <= 16 and T <= 80 throughout.
Case = namedtuple("Case", "id maps A P T E seed env_map")

CASES = [
    Case("P1", (M1,), 1, 1, 30, 8, 116, None),          # one robot, one package: list = 2
    Case("PK", (M1,), 8, 5, 25, 8, 200, None),          # P <= k: all spawn at t = 0, list = 2P
    Case("P64", (M1,), 8, 64, 40, 8, 428, None),        # last shape on the bpermute path, list 73 (two trips)
    Case("P65", (M3,), 5, 65, 40, 8, 400, None),        # first shape on the global-load path
    Case("P128", (S64,), 16, 128, 60, 6, 500, None),    # tj >= 64, the 16-robot engine, 64x64 tables
    Case("P129", (M3,), 21, 129, 40, 6, 984, None),     # k = 21, list > 128, three append chunks
    Case("A19", (M3,), 19, 60, 30, 8, 700, None),       # k = 20
    Case("A20", (M3,), 20, 60, 30, 8, 800, None),       # k = 21
    Case("A64", (S64,), 64, 257, 50, 5, 900, None),     # every lane a robot, five append chunks
    Case("ROOMS", ("rooms",), 4, 30, 60, 12, 1000, None),     # unreachable goals
    Case("ROOMS65", ("rooms",), 6, 65, 60, 8, 1100, None),    # ... on the global-load path
    Case("ROW", ("row",), 2, 5, 20, 8, 1200, None),     # only L / R neighbours in bounds
    Case("COL", ("col",), 3, 4, 25, 8, 1300, None),     # only U / D neighbours in bounds
    Case("SERP", ("serp",), 5, 20, 80, 16, 1416, None),  # BFS depth > 1,024
    # synthetic64 first: its table is the largest and lies at offset 0
    Case("MIX", (S64, M1, M2, M3), 5, 40, 80, 16, 1500, (0,) * 4 + (1,) * 4 + (2,) * 4 + (3,) * 4),
]
BY_ID = {c.id: c for c in CASES}


# ---- the synthetic maps
def rooms_grid():
    """9 x 13, a wall down column 6: two rooms of 9 x 6 with no door."""
    g = np.zeros((9, 13), np.uint8)
    g[:, 6] = 1
    return g


def serpentine_grid(n=64):
    """n x n, all wall but the odd rows (corridors over the whole width) and one cell of each even
    row between two corridors, alternately in the last and the first column: one long path."""
    g = np.ones((n, n), np.uint8)
    g[1::2, :] = 0
    for i, r in enumerate(range(2, n - 1, 2)):
        g[r, n - 1 if i % 2 == 0 else 0] = 0
    return g


SYNTHETIC = {"rooms": rooms_grid, "serp": serpentine_grid,
             "row": lambda: np.zeros((1, 12), np.uint8), "col": lambda: np.zeros((9, 1), np.uint8)}


def case_grids(case):
    return [SYNTHETIC[m]() if m in SYNTHETIC else grid(m) for m in case.maps]


def case_env_map(case):
    return np.zeros(case.E, np.int32) if case.env_map is None else np.asarray(case.env_map, np.int32)


def spawn_k(A):
    """Packages that spawn at t = 0 (where P allows)."""
    return min(A, 20) + 1


def components(g):
    """Labels of the 4-connected components of the free cells (walls -1), by min-propagation."""
    H, W = g.shape
    free = g == 0
    big = H * W
    lab = np.where(free, np.arange(big).reshape(H, W), big)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        m = np.minimum.reduce([lab, p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]])
        m = np.where(free, m, big)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(free, lab, -1)


def bfs_from(g, goal):
    """run_bfs's distance field from ``goal`` (r, c); -1 = not reached."""
    H, W = g.shape
    d = -np.ones((H, W), np.int64)
    d[goal] = 0
    q = deque([goal])
    while q:
        r, c = q.popleft()
        for nr, nc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
            if 0 <= nr < H and 0 <= nc < W and d[nr, nc] < 0 and g[nr, nc] == 0:
                d[nr, nc] = d[r, c] + 1
                q.append((nr, nc))
    return d


# ---- the agent record in a checkpoint (csrc/mdl_greedy.hip greedy_rec, csrc/mdl_engine.hip greedy_stride)
def record_layout(A, P):
    cap = 3 * P + 64
    list_off = (8 + 4 * A + 3) & ~3
    free_off = list_off + 2 * cap
    return dict(cap=cap, list_off=list_off, free_off=free_off, stride=(free_off + cap + 15) & ~15)


def record_rows(blob, E, A, P):
    """The raw agent records, uint8 [E, stride]: the tail of a checkpoint taken after greedy_init."""
    stride = record_layout(A, P)["stride"]
    return np.asarray(blob, np.uint8)[-E * stride:].reshape(E, stride)


def decode_record(row, A, P):
    L = record_layout(A, P)
    n, flags = (int(x) for x in row[:8].view(np.int32))
    assert 0 <= n <= L["cap"], f"record n = {n} outside [0, {L['cap']}]"
    return dict(n=n, flags=flags, target=row[8:8 + 2 * A].view(np.int16).astype(np.int32),
                prev_carry=row[8 + 2 * A:8 + 4 * A].view(np.int16).astype(np.int32),
                list=row[L["list_off"]:L["list_off"] + 2 * n].view(np.uint16).astype(np.int32),
                free=row[L["free_off"]:L["free_off"] + n].copy())


def assert_record(row, want, A, P, where):
    """A device record (raw row) against OracleGreedy.record()."""
    got = decode_record(row, A, P)
    assert got["n"] == want["n"], f"n {got['n']} != {want['n']}, {where}"
    assert got["flags"] == 0, f"flags {got['flags']}, {where}"
    np.testing.assert_array_equal(got["target"], want["target"], err_msg=f"target, {where}")
    np.testing.assert_array_equal(got["prev_carry"], want["carrying"], err_msg=f"prev_carry, {where}")
    np.testing.assert_array_equal(got["list"], want["list"], err_msg=f"list, {where}")
    np.testing.assert_array_equal(got["free"], want["free"], err_msg=f"free, {where}")


# ---- the oracle side
class OracleSide:
    """One OracleEnv + OracleGreedy per env; the agent is re-made at every episode end, as the
    reference's evaluation loop makes a new GreedyAgents per episode."""

    def __init__(self, case, probe=None):
        self.case = case
        self.grids = case_grids(case)
        self.env_map = case_env_map(case)
        self.probe = probe
        self.envs, self.agents = [], []
        for e in range(case.E):
            o = O.OracleEnv(self.grids[self.env_map[e]], case.A, case.P, case.T, seed=case.seed + e)
            o.reset()
            self.envs.append(o)
            self.agents.append(O.OracleGreedy(o))
            if probe is not None:
                probe.after_init(self, e)

    def seeds(self):
        return [self.case.seed + e for e in range(self.case.E)]

    def record(self, e):
        return self.agents[e].record()

    def actions(self, e):
        """get_actions of env e's agent: packed codes move | op << 3, uint8 [A]."""
        before = self.record(e) if self.probe is not None else None
        mv, op = self.agents[e].actions(self.envs[e])
        if self.probe is not None:
            self.probe.after_actions(self, e, before, mv, op)
        return (mv | (op << 3)).astype(np.uint8)

    def step(self, e, codes, auto_reset):
        """Steps env e; at an episode end with auto_reset the env is reset and its agent re-made."""
        r, _, done = self.envs[e].step(codes & 7, codes >> 3)
        if self.probe is not None:
            self.probe.after_step(self, e, r, done)
        if done and auto_reset:
            self.envs[e].reset()
            self.agents[e] = O.OracleGreedy(self.envs[e])
            if self.probe is not None:
                self.probe.after_init(self, e)
        return done


class Probe:
    """What a run of the oracle reached (test_greedy_matrix_cpu.py pins it per case)."""

    def __init__(self, case):
        self.case = case
        g = case_grids(case)
        self.comp = [components(x) for x in g]
        self.moves, self.ops = set(), set()
        self.max_n = 0
        self.deliveries = np.zeros(len(g), np.int64)       # per map group
        self.tj_ge64 = self.spawn_gt64 = self.other_comp = self.shifted = 0
        self.tie = self.not_lowest = self.choices = 0
        self.tj_max = -1                                   # highest package record a target named
        self.pick_max = -1                                 # highest list index a closest-free choice took
        self.far = 0                                       # BFS lookups with distance > 1,024
        self.far_wanted = False
        self.overflow = 0                                  # n > P + k

    def _n(self, n):
        self.max_n = max(self.max_n, n)
        self.overflow += n > self.case.P + spawn_k(self.case.A)

    def after_init(self, side, e):
        rec = side.record(e)
        self._n(rec["n"])
        self.spawn_gt64 += int((rec["list"] > 64).sum())

    def after_step(self, side, e, r, done):
        self.deliveries[side.env_map[e]] += r >= 0.5       # a delivery adds >= delay_reward (1.0)

    def after_actions(self, side, e, before, mv, op):
        c = self.case
        rec, st = side.record(e), side.envs[e].state()
        g, comp = side.grids[side.env_map[e]], self.comp[side.env_map[e]]
        rob, pk = st["robots"], st["pkgs"]
        self.moves.update(int(x) for x in mv)
        self.ops.update(int(x) for x in op)
        self._n(rec["n"])
        lst = rec["list"]
        self.spawn_gt64 += int((lst[before["n"]:] > 64).sum())
        # the choices, replayed: free flags as get_actions sees them, robot by robot
        free = np.concatenate([before["free"], np.ones(rec["n"] - before["n"], np.uint8)])
        start = pk[lst - 1, 0:2]
        for i in range(c.A):
            tgt = before["target"][i]
            if before["carrying"][i] != 0:                 # update_inner_state
                tgt = rob[i, 2]
            if tgt == 0 and free.any():
                d = np.abs(start - rob[i, 0:2]).sum(axis=1)
                cand = np.nonzero(free)[0]
                j = cand[np.argmin(d[cand])]               # argmin keeps the first
                assert lst[j] == rec["target"][i], "the replayed choice is the agent's"
                tied = cand[d[cand] == d[j]]
                self.choices += 1
                self.tie += len(set(lst[tied])) > 1        # tied entries that name different packages
                self.not_lowest += j != cand[0]
                self.pick_max = max(self.pick_max, int(j))
                free[lst[j] - 1] = 0
            t = rec["target"][i]
            if t == 0:
                continue
            tj = lst[t - 1] - 1
            self.tj_ge64 += tj >= 64
            self.tj_max = max(self.tj_max, int(tj))
            self.shifted += lst[t - 1] != t
            goal = tuple(pk[tj, 2:4] if rob[i, 2] != 0 else pk[tj, 0:2])
            here = tuple(rob[i, 0:2])
            self.other_comp += comp[goal] != comp[here]
            if self.far_wanted and not self.far and goal != here:
                self.far += bfs_from(g, goal)[here] > 1024
        np.testing.assert_array_equal(free, rec["free"], err_msg="the replayed free flags are the agent's")


def run_full(side, steps, dev=None, first=0):
    """The full-batch drive: every env acts, steps with auto-reset, and has its agent re-made at its
    episode end.  ``dev`` (None: the oracle alone) is the device side: actions() -> codes [E, A],
    check(side, where) compares the records, step(codes) -> done [E], reinit(ids)."""
    E = side.case.E
    for k in range(first, first + steps):
        want = np.stack([side.actions(e) for e in range(E)])
        if dev is not None:
            got = dev.actions()
            for e in range(E):
                np.testing.assert_array_equal(got[e] & 7, want[e] & 7, err_msg=f"move, env {e} step {k}")
                np.testing.assert_array_equal(got[e] >> 3, want[e] >> 3, err_msg=f"op, env {e} step {k}")
            dev.check(side, f"step {k}")
        done = np.array([side.step(e, want[e], True) for e in range(E)])
        if dev is not None:
            np.testing.assert_array_equal(dev.step(want), done, err_msg=f"done, step {k}")
            if done.any():
                dev.reinit(np.nonzero(done)[0])
                dev.check(side, f"re-initialised after step {k}")
