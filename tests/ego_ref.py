"""The reference rule of the robot-centred actor-map windows (BatchedEnv.build_obs_ego), the cases of
test_gpu_ego.py and their input conditions, computed from the oracle alone.

The rule: the window is a crop of the reference's own convert_observation tensor around the robot's cell
(the single 1 of channel 1), padded with ones in channel 0 (an off-map cell cannot be entered) and zeros
in channels 1-5.

Driving, as obs_ref: odd-numbered envs follow OracleGreedy (re-made every episode), so packages are
picked up and carried towards their targets; the even ones draw uniform trainer ints.  One OracleBatch
per env at seed + env id: the engine's own seeds.

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import oracle as O
from golden_io import grid
from obs_ref import _MOVE_TO_INT

ST_WAITING, ST_IN_TRANSIT = 1, 2


def ego_from_full(full, R):
    """full [.., A, 6, H, W] -> [.., A, 6, K, K], K = 2R + 1: each robot's window of its own map."""
    full = np.asarray(full)
    H, W = full.shape[-2:]
    K = 2 * R + 1
    flat = full.reshape(-1, 6, H, W)
    pad = np.zeros((flat.shape[0], 6, H + 2 * R, W + 2 * R), full.dtype)
    pad[:, 0] = 1
    pad[:, :, R:R + H, R:R + W] = flat
    out = np.empty((flat.shape[0], 6, K, K), full.dtype)
    for k in range(flat.shape[0]):
        pos = np.argwhere(flat[k, 1] == 1)
        assert len(pos) == 1, "channel 1 holds the robot's cell alone"
        r, c = pos[0]
        out[k] = pad[k, :, r:r + K, c:c + K]
    return out.reshape(full.shape[:-2] + (K, K))


# fixture maps built here: name -> (H, W, obstacle cells)
BUILT = {"line1x12": (1, 12, ((0, 5),)), "line9x1": (9, 1, ())}


def built_grid(name):
    H, W, walls = BUILT[name]
    g = np.zeros((H, W), np.uint8)
    for r, c in walls:
        g[r, c] = 1
    return g


# radii: every radius the case is built at; steps <= 25 with an auto-reset at T (and 2T);
# env_map: None, or the map of each env (contiguous groups)
Case = namedtuple("Case", "id maps A P T tracker radii E seed steps env_map")
M0, M1, M2, S64 = "map.txt", "map1.txt", "map2.txt", "synthetic64.txt"


def _c(id, maps, A, P, T, tracker, radii, E, seed=42, steps=25, env_map=None):
    return Case(id, (maps,) if isinstance(maps, str) else tuple(maps), A, P, T, tracker, tuple(radii), E, seed, steps,
                env_map)


CASES = [
    # 1. odd A: an env row is 24 * 5 * K^2 bytes, every second one only 8-B aligned
    _c("m1_a5_stale", M1, 5, 20, 10, "mappo", (1, 2), 8),
    _c("m1_a5_fresh", M1, 5, 20, 10, "fresh", (1, 2), 7),
    # 2. the window wider than the map; one-row and one-column maps
    _c("m7_wide_stale", M0, 4, 12, 10, "mappo", (5, 15), 8),
    _c("m7_wide_fresh", M0, 4, 12, 10, "fresh", (5, 15), 5),
    _c("line1x12", "line1x12", 3, 6, 10, "mappo", (2,), 8),
    _c("line9x1", "line9x1", 2, 5, 10, "fresh", (2,), 8),
    # 3. 20x20: map rows start in mid-word
    _c("m20_a8_stale", M2, 8, 30, 10, "mappo", (3,), 8),
    _c("m20_a8_fresh", M2, 8, 30, 10, "fresh", (3,), 6),
    # 4. 64x64: two words per map row, windows across column 32
    _c("s64_a16_stale", S64, 16, 100, 12, "mappo", (5, 15), 8),
    _c("s64_a16_fresh", S64, 16, 100, 12, "fresh", (5, 15), 4),
    # 5. no other robot; the robot groups (A = 64, R = 15: the image of all robots is 46 KB)
    _c("m1_a1", M1, 1, 8, 10, "mappo", (2,), 8),
    _c("s64_a64_groups", S64, 64, 100, 12, "mappo", (15,), 3),
    # 6. one engine over three map shapes; the tests also build one range across both boundaries
    _c("mixed_stale", (M1, M2, M0), 4, 12, 10, "mappo", (2, 5), 8, env_map=(0, 0, 0, 1, 1, 2, 2, 2)),
    _c("mixed_fresh", (M1, M2, M0), 4, 12, 10, "fresh", (3,), 7, env_map=(0, 0, 1, 1, 1, 2, 2)),
]
BY_ID = {c.id: c for c in CASES}


def grids(case):
    return [built_grid(m) if m in BUILT else grid(m) for m in case.maps]


def env_maps(case):
    return [0] * case.E if case.env_map is None else list(case.env_map)


def build_points(case):
    """After reset (-1), every third step, the auto-reset steps (the state is the new episode's first)
    and the step after each, and the last."""
    n, T = case.steps, case.T
    pts = {-1, n - 1} | {k for k in range(n) if k % 3 == 2}
    for r in range(1, n // T + 1):
        pts |= {r * T - 1, r * T}
    return sorted(k for k in pts if -1 <= k < n)


class Driver:
    def __init__(self, case):
        self.case = case
        self.gr = grids(case)
        em = env_maps(case)
        kw = dict(clear_on_reset=(case.tracker == "fresh"))
        self.b = [O.OracleBatch(1, self.gr[em[e]], case.A, case.P, case.T, seed_base=case.seed + e, **kw)
                  for e in range(case.E)]
        self.rs = np.random.RandomState(case.seed + 1000)
        self.greedy = {e: O.OracleGreedy(self.b[e].env(0)) for e in range(1, case.E, 2)}

    def actions(self):
        c = self.case
        ints = self.rs.randint(0, 15, size=(c.E, c.A)).astype(np.uint8)
        for e, ag in self.greedy.items():
            mv, op = ag.actions(self.b[e].env(0))
            ints[e] = _MOVE_TO_INT[mv] + 5 * op
        return ints

    def step(self, ints):
        dn = np.zeros(self.case.E, bool)
        for e, ob in enumerate(self.b):
            dn[e] = ob.step(ints[e:e + 1], auto_reset=True, consts=O.MAPPO_CONSTS)[2][0]
        for e in self.greedy:
            if dn[e]:
                self.greedy[e] = O.OracleGreedy(self.b[e].env(0))
        return dn

    def full(self):
        """The oracle's actor_map of every env: a list of [A, 6, H, W] (the maps may differ in shape)."""
        c = self.case
        return [ob.obs(c.T, max(c.A - 1, 0), 5, 4, 4)["actor_map"][0] for ob in self.b]

    def rows(self, e):
        """(t, robots [A, 3] 0-based, tracker rows [n, 8], package table [P, 8]) of env e."""
        st = self.b[e].env(0).state()
        return st["t"], st["robots"], self.b[e].tracker(0).rows(), st["pkgs"]


@functools.lru_cache(maxsize=None)
def trace(case):
    """The case on the oracle: [(k, ints or None, done or None, full or None)] for k = -1 (after reset),
    0 .. steps-1; full (Driver.full) at the build points."""
    d = Driver(case)
    pts = set(build_points(case))
    out = [(-1, None, None, d.full())]
    for k in range(case.steps):
        ints = d.actions()
        dn = d.step(ints)
        out.append((k, ints, dn, d.full() if k in pts else None))
    return out


CONDITIONS = ("top", "bottom", "left", "right", "corner", "other", "start", "target", "carried_in", "carried_out",
              "survivor")


@functools.lru_cache(maxsize=None)
def conditions(case, R):
    """How many windows of the case's build points (radius R) meet each input condition."""
    d = Driver(case)
    pts = set(build_points(case))
    c = dict.fromkeys(CONDITIONS, 0)
    c["resets"] = c["windows"] = 0

    def count():
        for e, full in enumerate(d.full()):
            H, W = full.shape[-2:]
            ego = ego_from_full(full, R)
            t, rob, rows, pk = d.rows(e)
            # survivors of an earlier episode: the tracker's row differs from the env's package of that id
            sv3, sv4 = [], []
            for x in rows:
                if tuple(x[2:8]) != tuple(pk[int(x[0]) - 1][0:6]):
                    waiting = x[1] == ST_WAITING and x[6] <= t
                    if waiting:
                        sv3.append((int(x[2]), int(x[3])))
                    if waiting or x[1] == ST_IN_TRANSIT:
                        sv4.append((int(x[4]), int(x[5])))
            for a in range(case.A):
                r, cc = (int(v) for v in rob[a, :2])
                assert full[a, 1, r, cc] == 1
                top, bottom, left, right = r - R < 0, r + R >= H, cc - R < 0, cc + R >= W
                c["windows"] += 1
                c["top"] += top
                c["bottom"] += bottom
                c["left"] += left
                c["right"] += right
                c["corner"] += (top or bottom) and (left or right)
                c["other"] += bool(ego[a, 2].any())
                c["start"] += bool(ego[a, 3].any())
                c["target"] += bool(ego[a, 4].any())
                c["carried_in"] += bool(ego[a, 5].any())
                c["carried_out"] += bool(rob[a, 2] != 0 and full[a, 5].any() and not ego[a, 5].any())
                for ch, cells in ((3, sv3), (4, sv4)):
                    for sr, sc in cells:
                        assert full[a, ch, sr, sc] == 1
                        c["survivor"] += abs(sr - r) <= R and abs(sc - cc) <= R

    count()
    for k in range(case.steps):
        c["resets"] += int(d.step(d.actions()).sum())
        if k in pts:
            count()
    return c


def expected(case, R):
    """The conditions the case must meet at radius R: all of them, less what its maps rule out -- no
    other robot with A = 1; a window leaves the map on a side only from a free cell within R of it
    (map1's border walls keep R = 1 inside); a carried target lies outside the window only if two free
    cells are more than R apart in a coordinate; survivors only with the stale tracker."""
    want = set(CONDITIONS)
    if case.A == 1:
        want.discard("other")
    if case.tracker != "mappo":
        want.discard("survivor")
    can = dict.fromkeys(("top", "bottom", "left", "right", "corner", "carried_out"), False)
    for g in grids(case):
        H, W = g.shape
        r, c = np.nonzero(g == 0)
        top, bottom, left, right = r - R < 0, r + R >= H, c - R < 0, c + R >= W
        for k, v in (("top", top), ("bottom", bottom), ("left", left), ("right", right),
                     ("corner", (top | bottom) & (left | right))):
            can[k] |= bool(v.any())
        can["carried_out"] |= bool(r.max() - r.min() > R or c.max() - c.min() > R)
    return want - {k for k, v in can.items() if not v}
