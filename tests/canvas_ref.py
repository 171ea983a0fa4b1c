"""The reference rule of the critic map on a fixed canvas (BatchedEnv.build_obs_canvas), the cases of
test_gpu_canvas.py / test_gpu_canvas_collect.py and their input conditions, computed from the oracle alone.

The rule: the canvas holds the reference's own convert_global_state map in its top-left [:H, :W] corner;
elsewhere channel 0 is 1 (an off-map cell cannot be entered) and channels 1-3 are 0.

Driving, as ego_ref: odd-numbered envs follow OracleGreedy (re-made every episode), so packages are picked
up and carried; the even ones draw uniform trainer ints.  One OracleBatch per env at seed + env id: the
engine's own seeds.  Replay steps the same oracle envs with a recorded action tensor (a collector's).

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import ego_ref as G
import oracle as O
from obs_ref import _MOVE_TO_INT

ST_WAITING, ST_IN_TRANSIT = 1, 2
MR = MPS = 4   # max_robots_state / max_packages_state of every case
MP = 5         # max_packages_obs
KEYS = ("actor_vec", "critic_map", "critic_vec")


def canvas_from_full(critic_map, Hc, Wc):
    """critic_map [.., 4, H, W] -> [.., 4, Hc, Wc]: the map in the top-left corner, obstacles around it."""
    cm = np.asarray(critic_map)
    H, W = cm.shape[-2:]
    assert Hc >= H and Wc >= W, "no cropping"
    out = np.zeros(cm.shape[:-3] + (4, Hc, Wc), cm.dtype)
    out[..., 0, :, :] = 1
    out[..., :, :H, :W] = cm
    return out


# steps <= 25 with an auto-reset at T (and 2T); env_map: None, or the map of each env (contiguous groups)
Case = namedtuple("Case", "id maps A P T tracker canvas E seed steps env_map")
M0, M1, M2, S64 = G.M0, G.M1, G.M2, G.S64


def _c(id, maps, A, P, T, tracker, canvas, E, seed=42, steps=25, env_map=None):
    return Case(id, (maps,) if isinstance(maps, str) else tuple(maps), A, P, T, tracker, tuple(canvas), E, seed, steps,
                env_map)


MIXED_MAP = (0, 0, 0, 1, 1, 2, 2, 2)
CASES = [
    # the pad inside the row's own word (a 13-bit canvas row holds the map's 10 bits)
    _c("m1_pad_stale", M1, 5, 20, 10, "mappo", (12, 13), 6),
    _c("m1_pad_fresh", M1, 5, 20, 10, "fresh", (12, 13), 5),
    # rows starting mid-word; odd Hc * Wc: every second env's half-type row is 8-byte aligned only
    _c("m20_id", M2, 8, 30, 10, "mappo", (20, 20), 5),
    _c("m20_odd", M2, 8, 30, 10, "mappo", (21, 23), 5),
    # one-row and one-column maps in one engine: padding on one side only
    _c("lines", ("line1x12", "line9x1"), 2, 5, 10, "mappo", (9, 12), 6, env_map=(0, 0, 0, 1, 1, 1)),
    # two words per map row; an 8-word canvas row, the largest Wc
    _c("s64_id", S64, 16, 100, 12, "mappo", (64, 64), 4, steps=14),
    _c("s64_wide", S64, 16, 100, 12, "fresh", (64, 255), 3, steps=14),
    # the 8 KB image at MDL_MAX_CELLS
    _c("big", M1, 5, 20, 10, "mappo", (128, 128), 3, steps=12),
    # one launch across both shape boundaries, the vector runs, identity for the middle group
    _c("mixed_stale", (M1, M2, M0), 4, 12, 10, "mappo", (20, 20), 8, env_map=MIXED_MAP),
    _c("mixed_stale_odd", (M1, M2, M0), 4, 12, 10, "mappo", (21, 23), 8, env_map=MIXED_MAP),
    _c("mixed_fresh", (M1, M2, M0), 4, 12, 10, "fresh", (20, 20), 8, env_map=MIXED_MAP),
    _c("mixed_fresh_odd", (M1, M2, M0), 4, 12, 10, "fresh", (21, 23), 8, env_map=MIXED_MAP),
    # more than one workgroup, and a partial one
    _c("e67", M1, 5, 20, 10, "mappo", (12, 13), 67, steps=4),
]
BY_ID = {c.id: c for c in CASES}
MIXED = tuple(c for c in CASES if c.env_map == MIXED_MAP)


def base(case):
    """The case less its id and canvas: what the oracle trace depends on (cases that differ in the canvas
    alone share one trace)."""
    return case._replace(id="", canvas=())


grids = G.grids
env_maps = G.env_maps
build_points = G.build_points


def shapes(case):
    """(H, W) of every env's map."""
    g = grids(case)
    return [g[m].shape for m in env_maps(case)]


class Driver:
    """One OracleBatch per env at seed + e.  consts / auto_reset: the MAPPO rollout's by default."""

    def __init__(self, case, consts=None, auto_reset=True):
        self.case = case
        self.gr = grids(case)
        em = env_maps(case)
        self.consts = O.MAPPO_CONSTS if consts is None else consts
        self.auto_reset = auto_reset
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

    def step(self, ints, running=None):
        """Step every env (or those `running` marks) with ints [E, A] -> (r_env f64, r_shaped f32, done) [E],
        zeros where not stepped."""
        E = self.case.E
        r, sh, dn = np.zeros(E, np.float64), np.zeros(E, np.float32), np.zeros(E, bool)
        for e, ob in enumerate(self.b):
            if running is None or running[e]:
                a, b, c = ob.step(np.asarray(ints[e:e + 1], np.uint8), auto_reset=self.auto_reset, consts=self.consts)
                r[e], sh[e], dn[e] = a[0], b[0], c[0]
        for e in self.greedy:
            if dn[e] and self.auto_reset:
                self.greedy[e] = O.OracleGreedy(self.b[e].env(0))
        return r, sh, dn

    def obs(self, e):
        """The oracle's four tensors of env e (no leading env axis)."""
        c = self.case
        o = self.b[e].obs(c.T, max(c.A - 1, 0), MP, MR, MPS)
        return {k: v[0] for k, v in o.items()}

    def obs_all(self):
        return [self.obs(e) for e in range(self.case.E)]

    def rows(self, e):
        """(t, robots [A, 3] 0-based, tracker rows [n, 8], package table [P, 8]) of env e."""
        st = self.b[e].env(0).state()
        return st["t"], st["robots"], self.b[e].tracker(0).rows(), st["pkgs"]

    def state(self, e):
        return self.b[e].env(0).state()


def want(obs, canvas):
    """A list of per-env oracle observations -> the three arrays build_obs_canvas writes: actor_vec
    [E, A, Dv], critic_map [E, 4, Hc, Wc], critic_vec [E, Dg]."""
    return dict(actor_vec=np.stack([o["actor_vec"] for o in obs]),
                critic_map=np.stack([canvas_from_full(o["critic_map"], *canvas) for o in obs]),
                critic_vec=np.stack([o["critic_vec"] for o in obs]))


@functools.lru_cache(maxsize=None)
def trace(bcase):
    """base(case) on the oracle: [(k, ints or None, done or None, obs or None)] for k = -1 (after reset),
    0 .. steps-1; obs (Driver.obs_all) at the build points."""
    d = Driver(bcase)
    pts = set(build_points(bcase))
    out = [(-1, None, None, d.obs_all())]
    for k in range(bcase.steps):
        ints = d.actions()
        dn = d.step(ints)[2]
        out.append((k, ints, dn, d.obs_all() if k in pts else None))
    return out


CONDITIONS = ("robot_last_row", "robot_last_col", "start_last_row", "start_last_col", "target_last_row",
              "target_last_col", "survivor", "not_started", "carried")


@functools.lru_cache(maxsize=None)
def conditions(bcase):
    """How many (build point, env) pairs of the case meet each input condition.  The last-row conditions
    count only envs whose canvas pads below the map, the last-column ones those it pads to the right of --
    they are asked of padded cases (conditions_of)."""
    d = Driver(bcase)
    pts = set(build_points(bcase))
    c = dict.fromkeys(CONDITIONS, 0)
    c["resets"] = 0

    def count():
        for e in range(bcase.E):
            cm = d.obs(e)["critic_map"]
            H, W = cm.shape[-2:]
            t, rob, rows, pk = d.rows(e)
            for name, ch in (("robot", 1), ("start", 2), ("target", 3)):
                c[name + "_last_row"] += bool(cm[ch, H - 1, :].any())
                c[name + "_last_col"] += bool(cm[ch, :, W - 1].any())
            for x in rows:
                shown = x[1] == ST_WAITING and x[6] <= t
                if tuple(x[2:8]) != tuple(pk[int(x[0]) - 1][0:6]) and (shown or x[1] == ST_IN_TRANSIT):
                    assert cm[3, int(x[4]), int(x[5])] == 1   # a survivor of an earlier episode, on the map
                    c["survivor"] += 1
                if x[1] == ST_WAITING and x[6] > t:
                    c["not_started"] += 1
                    if not any(y[1] == ST_WAITING and y[6] <= t and tuple(y[2:4]) == tuple(x[2:4]) for y in rows):
                        assert cm[2, int(x[2]), int(x[3])] == 0   # channel 2 does not show it
            for a in range(bcase.A):
                if rob[a, 2] != 0:
                    it = [x for x in rows if int(x[0]) == int(rob[a, 2]) and x[1] == ST_IN_TRANSIT]
                    if it:
                        assert cm[3, int(it[0][4]), int(it[0][5])] == 1   # channel 3 from an in-transit entry
                        c["carried"] += 1

    count()
    for k in range(bcase.steps):
        c["resets"] += int(d.step(d.actions())[2].sum())
        if k in pts:
            count()
    return c


class Replay:
    """The oracle stepped with a recorded action tensor: Driver without its own actions."""

    def __init__(self, case, consts=None, auto_reset=True):
        self.d = Driver(case, consts=consts, auto_reset=auto_reset)
        self.d.greedy = {}

    def step(self, ints, running=None):
        return self.d.step(np.asarray(ints, np.uint8), running)

    def obs_all(self):
        return self.d.obs_all()

    def obs(self, e):
        return self.d.obs(e)

    def total_reward(self, e):
        return self.d.state(e)["total_reward"]
