"""The oracle side of tests/launch_matrix.py, shared by tests/test_host_cpu.py (the input conditions
alone) and tests/test_gpu_launch_matrix.py (the device side against it).  No GPU here.

Every run is a list of calls, each with what the engine must hold after it: the state of all E envs
(robots, packages, t, total reward, tracker rows), so an env the call does not name must come out
unchanged.  Each env is its own single-env OracleBatch with seed + e, which lets one engine mix maps."""
import numpy as np

import oracle as O
from golden_io import grid

REFILL = 624   # MT19937 words per refill


class Envs:
    """E oracle envs, one per engine env; grids: one grid or one per env."""

    def __init__(self, grids, E, A, P, T, seed, tracker, constructed=False):
        self.grids = [grids] * E if isinstance(grids, np.ndarray) else list(grids)
        self.E, self.A, self.P, self.T, self.fresh = E, A, P, T, tracker == "fresh"
        if constructed:   # Environment() alone: the constructor's layout draw (what k_seed leaves).  The stale
            self.b = None  # tracker is still empty; the fresh one is the env's own truth at every moment
            self.envs = [O.OracleEnv(self.grids[e], A, P, T, seed=seed + e) for e in range(E)]
            self.trks = [O.OracleTracker(max(P, 1)) for _ in range(E)]
            if self.fresh:
                for k, x in zip(self.trks, self.envs):
                    k.update_from_env(x)
        else:             # ... then reset() and the tracker's first update
            self.b = [O.OracleBatch(1, self.grids[e], A, P, T, seed_base=seed + e, clear_on_reset=self.fresh)
                      for e in range(E)]
            self.envs = [b.env(0) for b in self.b]
            self.trks = [b.tracker(0) for b in self.b]

    def step(self, ints, auto_reset):
        out = [b.step(ints[e:e + 1], auto_reset=auto_reset, consts=O.MAPPO_CONSTS) for e, b in enumerate(self.b)]
        return tuple(np.concatenate([o[k] for o in out]) for k in range(3))

    def reset(self, ids):
        """Environment.reset() of the listed envs, tracker.clear() in fresh mode, then the update."""
        for e in ids:
            self.envs[e].reset()
            if self.fresh:
                self.trks[e].clear()
            self.trks[e].update_from_env(self.envs[e])

    def clear(self, ids):
        for e in ids:
            self.trks[e].clear()

    def state(self):
        st = [x.state() for x in self.envs]
        return dict(robots=np.stack([x["robots"] for x in st]), pkgs=np.stack([x["pkgs"] for x in st]),
                    t=np.array([x["t"] for x in st], np.int32),
                    total_reward=np.array([x["total_reward"] for x in st], np.float64),
                    rows=[k.rows() for k in self.trks])

    def counters(self):
        c = [x.counters() for x in self.envs]
        return {k: np.array([x[k] for x in c], np.int64) for k in ("words", "rejected", "retries")}

    def features(self, e, shape=None):
        """(idq_obs [A, 6, H, W], qmix_state [7, oh, ow]) of env e now."""
        g = self.grids[e]
        env = self.envs[e]
        t, r1, rows = env.state()["t"], env.robots1(), self.trks[e].rows()
        return (np.stack([O.idq_convert_state(g, t, r1, rows, a) for a in range(self.A)]),
                O.qmix_global_tensor(g, t, r1, rows, (7,) + g.shape if shape is None else shape))


def survivors(state, e):
    """Tracker rows of env e whose data is not that of the env's current package of the same id: entries
    left over from an earlier episode.  Returns (rows, those of them in transit)."""
    rows, pk = state["rows"][e], state["pkgs"][e]
    old = np.array([not np.array_equal(r[2:8], pk[r[0] - 1][0:6]) for r in rows], bool)
    return rows[old], rows[old & (rows[:, 1] == 2)] if len(rows) else rows[:0]


# ------------------------------------------------------------------ reset cases
def reset_ids(case):
    """The three explicit resets: (ids the engine is handed, ids that are reset)."""
    E = case.E
    desc = [e for e in reversed(range(E)) if e != 1]              # a host list of E - 1 ids, descending
    some = [1, 0, E - 1]                                          # env 1: its first reset, at t = T - 1
    if case.mail:                                                 # mail_reset takes host ids only
        return [(desc, desc), (some, some), (None, list(range(E)))]
    return [(desc, desc), ([1, E + 3, 0, E - 1], some), (None, list(range(E)))]   # E + 3: skipped on the device


def clear_ids(case):
    return [1, case.E - 2]


CLEAR_AT = (2, 5)   # the stale cases clear a subset's trackers mid-episode: third round, before its sixth step


def reset_trace(case, grids=None):
    """Calls of a seed or reset case: dicts with op (seed | reset | step | clear), what the engine is given
    (ids / ints), the results of a step (r, sh, done) and the state of all E envs after the call."""
    g = grid(case.map) if grids is None else grids
    args = (g, case.E, case.A, case.P, case.T, case.seed, case.tracker)
    trace = [dict(op="seed", state=Envs(*args, constructed=True).state())]
    orc = Envs(*args)
    trace.append(dict(op="reset", given=None, ids=list(range(case.E)), state=orc.state()))
    if case.kind == "seed":
        return trace
    rs = np.random.RandomState(case.rng)
    for rnd, (given, ids) in enumerate(reset_ids(case)):
        for k in range(case.rounds[rnd]):
            if case.tracker == "mappo" and (rnd, k) == CLEAR_AT:
                orc.clear(clear_ids(case))
                trace.append(dict(op="clear", ids=clear_ids(case), state=orc.state()))
            ints = rs.randint(0, 15, size=(case.E, case.A)).astype(np.uint8)
            r, sh, dn = orc.step(ints, False)
            trace.append(dict(op="step", ints=ints, r=r, sh=sh, done=dn, state=orc.state()))
        before = trace[-1]["state"]
        orc.reset(ids)
        trace.append(dict(op="reset", given=given, ids=ids, before=before, state=orc.state(), explicit=rnd + 1))
    return trace


def check_reset_inputs(case, trace):
    """The conditions on a reset case's inputs, from the oracle's trace alone."""
    assert [c["op"] for c in trace[:2]] == ["seed", "reset"]
    if case.kind == "seed":
        return
    assert not any(c["done"].any() for c in trace if c["op"] == "step"), "the rounds end before the time limit"
    resets = [c for c in trace if c.get("explicit")]
    assert [c["explicit"] for c in resets] == [1, 2, 3]
    assert any((c["state"]["robots"][:, :, 2] > 0).any() for c in trace), "no robot ever carries a package"
    if case.tracker != "mappo":
        return
    nch = next(k for k in (1, 2, 4, 8, 16) if case.P <= 64 * k)
    # a row that a reset finds in the tracker survives it: one in the upper half of the chunks
    high = any((c["before"]["rows"][e][:, 0] > 64 * nch // 2).any() for c in resets for e in c["ids"])
    for c in resets[1:]:
        st, ids = c["before"], c["ids"]
        assert any((st["rows"][e][:, 1] == 2).any() for e in ids), \
            f"reset {c['explicit']}: no reset env's tracker holds an in-transit row"
        assert any(len(survivors(st, e)[0]) for e in ids), \
            f"reset {c['explicit']}: no reset env's tracker holds a survivor of an earlier episode"
    assert nch == 1 or high, f"no surviving row has an id above {64 * nch // 2}"
    assert any(c["op"] == "clear" for c in trace)
    k = next(i for i, c in enumerate(trace) if c["op"] == "clear")
    assert any(len(trace[k - 1]["state"]["rows"][e]) for e in trace[k]["ids"]), "the cleared trackers were empty"


# ------------------------------------------------------------------ cycle cases
CYCLE_STEPS = (8, 4)   # steps before the "mixed" and before the "all" lazy reset


def cycle_masks(E):
    mixed = np.zeros(E, np.uint8)
    mixed[[0, 2, E - 2]] = 1
    return [mixed, np.ones(E, np.uint8)]


def cycle_trace(case, grids=None):
    """Calls of a cycle case: steps (op step) and lazy resets (op begin: mask, the finished episodes'
    return and length, the marked envs' observations) with the state of all E envs after each."""
    g = grid(case.map) if grids is None else grids
    orc = Envs(g, case.E, case.A, case.P, case.T, case.seed, "fresh")   # the trainer's constructor: empty tracker, reset
    rs = np.random.RandomState(case.rng + 5)
    trace = []
    for n, mask in zip(CYCLE_STEPS, cycle_masks(case.E)):
        for _ in range(n):
            ints = rs.randint(0, 15, size=(case.E, case.A)).astype(np.uint8)
            r, sh, dn = orc.step(ints, False)
            trace.append(dict(op="step", ints=ints, r=r, done=dn, state=orc.state()))
        st = orc.state()
        ids = np.nonzero(mask)[0].tolist()
        orc.clear(ids)
        orc.reset(ids)
        trace.append(dict(op="begin", mask=mask, ids=ids, ret=np.where(mask != 0, st["total_reward"], 0.0),
                          steps=np.where(mask != 0, st["t"], 0).astype(np.int32), state=orc.state(),
                          obs={e: orc.features(e) for e in ids}))
    return trace


def check_cycle_inputs(case, trace):
    begins = [c for c in trace if c["op"] == "begin"]
    assert [int(c["mask"].sum()) for c in begins] == [len(set([0, 2, case.E - 2])), case.E]
    assert all((c["steps"][c["ids"]] > 0).all() for c in begins) and any(c["ret"].any() for c in begins)
    k = trace.index(begins[0])
    off = [e for e in range(case.E) if e not in begins[0]["ids"]]
    assert off and any(len(trace[k - 1]["state"]["rows"][e]) for e in off)   # an unmarked env has rows to keep


# ------------------------------------------------------------------ alt cases
def alt_steps(case):
    return 2 * case.T + 3   # two auto-resets of every env and three steps of the third episode


def alt_trace(case, other_shape=None):
    """Calls of an alt case: op begin, then one step with auto-reset per call: the actions, the IDQ reward
    of every agent (reward_shaping on the state and tracker from before the step, ops as ints), done,
    the state after it and every env's observations (other: the qmix state at `other_shape`)."""
    g = grid(case.map)
    orc = Envs(g, case.E, case.A, case.P, case.T, case.seed, case.tracker)
    rs = np.random.RandomState(case.rng + 9)

    def obs():
        f = [orc.features(e) for e in range(case.E)]
        d = dict(idq=np.stack([x[0] for x in f]), qst=np.stack([x[1] for x in f]))
        if other_shape is not None:
            d["other"] = np.stack([orc.features(e, other_shape)[1] for e in range(case.E)])
        return d

    trace = [dict(op="begin", state=orc.state(), obs=obs())]
    for _ in range(alt_steps(case)):
        ints = rs.randint(0, 15, size=(case.E, case.A)).astype(np.uint8)
        pre = [(x.state()["t"], x.robots1(), k.rows()) for x, k in zip(orc.envs, orc.trks)]
        _, _, dn = orc.step(ints, True)
        op = np.where(ints // 5 >= 3, 0, ints // 5).astype(np.uint8)
        r = np.stack([O.idq_reward_shaping(pt, pr1, x.state()["t"], x.robots1(), op[e], True, rows, case.A)
                      for e, ((pt, pr1, rows), x) in enumerate(zip(pre, orc.envs))])
        trace.append(dict(op="step", ints=ints, r_idq=r, done=dn, state=orc.state(), obs=obs()))
    return trace


def check_alt_inputs(case, trace):
    n = np.zeros(case.E, np.int64)
    for c in trace[1:]:
        n += c["done"]
    assert (n >= 2).all(), "every env must pass two auto-resets"
    assert any(abs(c["r_idq"]).max() >= 2.0 for c in trace[1:]), "no pick-up or delivery is ever rewarded"
    if case.tracker == "mappo":
        sv = [survivors(c["state"], e) for c in trace for e in range(case.E)]
        assert any(len(a) for a, _ in sv), "no checked tracker holds a survivor of an earlier episode"
        assert any(len(b) for _, b in sv), "no checked tracker holds an in-transit survivor"


# ------------------------------------------------------------------ the reset storm
def _walled(H, W, free):
    """An H x W grid whose first `free` cells in row-major order are free, the others walls."""
    g = np.ones(H * W, np.uint8)
    g[:free] = 0
    return g.reshape(H, W)


# name: (grid, A, P, T, E, tracker, resets or None for "until every env has crossed three refills")
STORM = {
    "refills": (lambda: grid("map1.txt"), 1, 1, 25, 4, "fresh", None),
    "p1024": (lambda: grid("map3.txt"), 5, 1024, 25, 3, "mappo", 3),
    "rejections": (lambda: _walled(6, 6, 33), 5, 64, 25, 4, "fresh", 6),      # 2^5 + 1 free cells
    "two-cells": (lambda: _walled(3, 3, 2), 1, 20, 25, 4, "mappo", 6),
    "T2": (lambda: grid("map1.txt"), 5, 64, 2, 4, "fresh", 6),
    "full": (lambda: _walled(3, 3, 5), 5, 8, 25, 4, "mappo", 6),               # A = the number of free cells
}
STORM_SEED = 7


def storm_trace(name):
    """Explicit resets of all envs: per reset the state after it and the generator's counters
    (words, rejected, retries per env) before and after."""
    mk, A, P, T, E, tracker, n = STORM[name]
    orc = Envs(mk(), E, A, P, T, STORM_SEED, tracker)
    trace = []
    while len(trace) < (n or 10 ** 6):
        before = orc.counters()
        orc.reset(range(E))
        trace.append(dict(state=orc.state(), before=before, after=orc.counters()))
        if n is None and ((trace[-1]["after"]["words"] // REFILL - trace[0]["before"]["words"] // REFILL) >= 3).all():
            break
    return trace


def check_storm_inputs(name, trace):
    """What the oracle's counters must show for the storm case to reach its edge of the draw stream."""
    mk, A, P, T, E, tracker, n = STORM[name]
    F = int((mk() == 0).sum())
    d = {k: np.stack([c["after"][k] - c["before"][k] for c in trace]) for k in ("words", "rejected", "retries")}
    crossed = np.stack([c["after"]["words"] // REFILL - c["before"]["words"] // REFILL for c in trace])   # [reset, env]
    lim = min(A, 20)
    starts = max(0, P - lim - 1) if T > 2 else 0          # randint(1, 2) is one value: no draw
    robots = A - (1 if A == F else 0)                     # the last of F robots has one cell left: no draw
    # every accepted word is one of the reset's draws: robots, start and target (with its retries),
    # deadline, start time -- so a draw the shape rules out shows as a missing word
    assert (d["words"] - d["rejected"] == robots + 3 * P + d["retries"] + starts).all(), name
    if name == "refills":
        assert (A, P) == (1, 1) and (crossed.sum(0) >= 3).all(), crossed.sum(0)
    elif name == "p1024":
        assert P == 1024 and crossed.max() >= 5, crossed.max()
    elif name == "rejections":
        assert F - 1 == 1 << (F - 1).bit_length() - 1, F
        assert (4 * d["rejected"].sum(0) > d["words"].sum(0)).all(), (d["rejected"].sum(0), d["words"].sum(0))
    elif name == "two-cells":
        assert F == 2 and (d["retries"].sum(0) > 0).all()
    elif name == "T2":
        assert T == 2 and P > lim + 1 and starts == 0
    elif name == "full":
        assert A == F and robots == A - 1 and starts > 0
