"""Packed view records, batches of them and the oracle's answers, shared by tests/test_views_batch_cpu.py
(the conditions on the inputs alone) and tests/test_gpu_views_batch.py (the mdl_views_* entry points
against them).  No GPU here.

A transition is one oracle step: the state and tracker before it (the "prev" view record of
include/mdl_engine.h), the robots and time after it (the "cur" record), the actions and the global
reward.  All transitions are packed back to back into three blobs (prev records, cur records, action
bytes); a batch is a list of transitions, addressed through offsets into those blobs, with one agent
index per view.  Everything is cached and must be left unchanged by its users."""
import functools

import numpy as np

import oracle as O
from golden_io import decode_trainer, grid

ROBOTS = (1, 3, 5, 16)
PACKAGES = (1, 7, 20, 40, 12, 3, 33, 25)
T = 12              # the rollouts' episode length: every rollout passes two resets; also the builders' T
STEPS = 30
SNAP = range(1, STEPS, 4)       # the steps whose transition is kept
BATCH_N = (1, 5, 37)
TRUNCATING, PADDING = (2, 3, 2, 4), (30, 100, 50, 120)   # (MO, MP, MR, MPs)
TRAINER_INT = np.array([3, 1, 2, 4, 0], np.uint8)       # move code S L R U D -> the trainer's D L R S U index
CONSTS = {"mappo": O.MAPPO_CONSTS, "qmix": O.QMIX_CONSTS}

# (map, robots, packages, seed, tracker, greedy): per map every robot count in both tracker modes, half
# of them driven by the greedy agent
ROLLOUTS = [(m, ROBOTS[k % 4], PACKAGES[(k + 3 * m) % 8], 500 + 40 * m + k, ("fresh", "mappo")[k // 4],
             (k + k // 4) % 2 == 1) for m in range(4) for k in range(8)]


@functools.lru_cache(maxsize=None)
def maps():
    """The engine's maps: the 7x7 one, map1 (10x10), map1 mirrored, and map1 with inner walls.  map1 is an
    empty room, so its mirror image has the same walls: map 2 checks the per-view map index and offsets,
    and only map 3 tells a view read with another 10x10 map's walls from one read with its own."""
    g1 = grid("map1.txt")
    g3 = g1.copy()
    g3[3, 2:5] = 1
    g3[6, 6] = g3[7, 6] = g3[5, 1] = 1
    return grid("map.txt"), g1, np.ascontiguousarray(g1[:, ::-1]), g3


def _rollout(m, A, P, seed, tracker, greedy):
    g = maps()[m]
    fresh = tracker == "fresh"
    b = O.OracleBatch(1, g, A, P, T, seed_base=seed, clear_on_reset=fresh)
    env, trk = b.env(0), b.tracker(0)
    agent = O.OracleGreedy(env) if greedy else None
    rs = np.random.RandomState(seed)
    out = []
    for k in range(STEPS):
        if greedy:
            mv, op = agent.actions(env)
            ints = (TRAINER_INT[mv] + 5 * op).astype(np.uint8)
        else:
            ints = rs.randint(0, 15, size=A).astype(np.uint8)
            mv, op = decode_trainer(ints)
        s0, rows0 = env.state(), trk.rows()
        r, _, dn = b.step(ints[None], auto_reset=False)
        s1 = env.state()
        if k in SNAP:
            out.append(dict(map=m, A=A, t0=s0["t"], rob0=s0["robots"], rows0=rows0, t1=s1["t"], rob1=s1["robots"],
                            mv=mv.astype(np.uint8), op=op.astype(np.uint8), g=float(r[0]), greedy=greedy))
        if dn[0]:
            env.reset()
            if fresh:
                trk.clear()
            trk.update_from_env(env)
            if greedy:
                agent = O.OracleGreedy(env)
    return out


def _by_hand():
    """Two records no rollout is sure to give: an empty tracker, and one whose only slots are in transit."""
    f0, f2 = np.argwhere(maps()[0] == 0), np.argwhere(maps()[2] == 0)
    rob = np.array([[*f0[0], 0], [*f0[5], 0], [*f0[9], 0]], np.int32)
    empty = dict(map=0, A=3, t0=4, rob0=rob, rows0=np.zeros((0, 8), np.int32), t1=5, rob1=rob.copy(),
                 mv=np.zeros(3, np.uint8), op=np.array([0, 1, 2], np.uint8), g=-0.03, greedy=False)
    rob0 = np.array([[*f2[3], 0], [*f2[11], 9], [*f2[20], 0], [*f2[31], 2], [*f2[40], 0]], np.int32)
    rows = np.array([[9, 2, *f2[7], *f2[11], 1, 9], [2, 2, *f2[30], *f2[50], 0, 3]], np.int32)
    rob1 = rob0.copy()
    rob1[1, 2] = 0            # robot 1 stood on package 9's target and dropped it
    transit = dict(map=2, A=5, t0=6, rob0=rob0, rows0=rows, t1=7, rob1=rob1, mv=np.zeros(5, np.uint8),
                   op=np.array([0, 2, 1, 0, 2], np.uint8), g=9.95, greedy=False)
    return [empty, transit]


class Pool:
    """Every transition, and the three blobs with each transition's offsets into them."""

    def __init__(self, trans):
        self.trans = trans
        prev, cur, act = [], [], []
        self.prev_off, self.cur_off, self.act_off = (np.zeros(len(trans), np.int64) for _ in range(3))
        pw = cw = ab = 0
        for i, x in enumerate(trans):
            p = np.concatenate([[x["t0"], x["A"], len(x["rows0"]), x["map"]], x["rob0"].ravel(), x["rows0"].ravel()])
            c = np.concatenate([[x["t1"], x["A"]], x["rob1"].ravel()])
            self.prev_off[i], self.cur_off[i], self.act_off[i] = pw, cw, ab
            prev.append(p)
            cur.append(c)
            act.append(x["mv"] | (x["op"] << 3))
            pw, cw, ab = pw + p.size, cw + c.size, ab + x["A"]
        self.prev = np.concatenate(prev).astype(np.int32)
        self.cur = np.concatenate(cur).astype(np.int32)
        self.act = np.concatenate(act).astype(np.uint8)
        self.ns = np.array([len(x["rows0"]) for x in trans])
        self.A = np.array([x["A"] for x in trans])
        self.map = np.array([x["map"] for x in trans])
        self.g = np.array([x["g"] for x in trans], np.float64)


@functools.lru_cache(maxsize=None)
def pool():
    trans = [x for spec in ROLLOUTS for x in _rollout(*spec)]
    return Pool(trans + _by_hand())


class Batch:
    def __init__(self, name, idx, agent):
        p = pool()
        self.name, self.idx, self.agent = name, np.asarray(idx), np.asarray(agent, np.int32)
        self.n = len(idx)
        self.ns, self.A, self.map = p.ns[self.idx], p.A[self.idx], p.map[self.idx]
        self.max_slots = int(self.ns.max())
        self.shape = maps()[int(self.map[0])].shape      # of the first view: the features batches have one shape
        # IDQ ops / rewards: view w's A entries start at op_off[w], with gaps of 1..3 entries between views
        gaps = 1 + np.arange(self.n) % 3
        self.op_off = (np.cumsum(self.A + gaps) - self.A).astype(np.int64)
        self.op_total = int(self.op_off[-1] + self.A[-1])

    def sizes(self):
        """The three (MO, MP, MR, MPs): truncating, padding, and one between the batch's smallest and largest
        n_slots, so that one launch truncates some views and pads others."""
        lo, hi = int(self.ns.min()), int(self.ns.max())
        mid = (lo + hi + 1) // 2
        return [TRUNCATING, PADDING, (4, mid, 4, min(mid + 1, max(hi, 1)))]

    def ops(self):
        """The op bytes laid out at op_off (255, an op that matches nothing, in the gaps)."""
        out = np.full(self.op_total, 255, np.uint8)
        for w, i in enumerate(self.idx):
            out[self.op_off[w]:self.op_off[w] + self.A[w]] = pool().trans[i]["op"]
        return out


@functools.lru_cache(maxsize=None)
def batches():
    """name -> Batch.  "small-n" (map 0) / "large-n" (maps 1, 2 and 3 mixed): views of one map shape, which is
    what the feature builders take; "mixed-n": all maps (the reward entry points).  Every batch of five or
    more views holds the by-hand record of its shape and one agent index out of range on each side."""
    p = pool()
    rs = np.random.RandomState(20)
    hand = {0: len(p.trans) - 2, 2: len(p.trans) - 1}
    out = {}
    for kind, ms, forced in (("small", (0,), [hand[0]]), ("large", (1, 2, 3), [hand[2]]),
                             ("mixed", (0, 1, 2, 3), [hand[0], hand[2]])):
        cands = [i for i in range(len(p.trans) - 2) if p.map[i] in ms]
        for n in BATCH_N:
            idx = rs.choice(cands, n, replace=False)
            if n >= 5:
                idx[2:2 + len(forced)] = forced
            agent = np.array([rs.randint(0, p.A[i]) for i in idx], np.int32)
            if n >= 5:
                agent[1], agent[n - 2] = -1, p.A[idx[n - 2]]
            out[f"{kind}-{n}"] = Batch(f"{kind}-{n}", idx, agent)
    return out


FEATURE_BATCHES = [f"{k}-{n}" for k in ("small", "large") for n in BATCH_N]
REWARD_BATCHES = [f"mixed-{n}" for n in BATCH_N] + ["large-37"]


def _views(name):
    p = pool()
    b = batches()[name]
    for w, i in enumerate(b.idx):
        x = p.trans[i]
        r0, r1 = x["rob0"].copy(), x["rob1"].copy()
        r0[:, :2] += 1
        r1[:, :2] += 1
        yield w, x, maps()[x["map"]], r0, r1


@functools.lru_cache(maxsize=None)
def features(name, sizes):
    """obs [n, 6, H, W], vec [n, Dv], gmap [n, 4, H, W], gvec [n, Dg] of a features batch."""
    MO, MP, MR, MPs = sizes
    b = batches()[name]
    obs, vec, gmap, gvec = [], [], [], []
    for w, x, g, r0, _ in _views(name):
        a = int(b.agent[w])
        obs.append(O.convert_observation(g, x["t0"], r0, x["rows0"], a))
        vec.append(O.generate_vector_features(g.shape[0], g.shape[1], x["t0"], r0, x["rows0"], a, T, MO, MP))
        gm, gv = O.convert_global_state(g, x["t0"], r0, x["rows0"], T, MR, MPs)
        gmap.append(gm)
        gvec.append(gv)
    return dict(obs=np.stack(obs), vec=np.stack(vec), gmap=np.stack(gmap), gvec=np.stack(gvec))


@functools.lru_cache(maxsize=None)
def shaped(name, consts):
    """compute_shaped_rewards per transition, f32 [n]; consts: "mappo" or "qmix"."""
    return np.array([O.compute_shaped_rewards(x["g"], x["t0"], r0, x["t1"], r1, x["mv"], x["op"], x["rows0"], x["A"],
                                              CONSTS[consts]) for _, x, _, r0, r1 in _views(name)], np.float32)


def alt_shapes(name):
    """The two qmix state shapes of a features batch: the map's own and one padded in H, cropped in W."""
    H, W = batches()[name].shape
    return [(7, H, W), (7, H + 3, W - 2)]


@functools.lru_cache(maxsize=None)
def alt(name, shape):
    """idq_obs [n, 6, H, W] and qmix_state [n, 7, oh, ow] of a features batch."""
    b = batches()[name]
    idq = [O.idq_convert_state(g, x["t0"], r0, x["rows0"], int(b.agent[w])) for w, x, g, r0, _ in _views(name)]
    qst = [O.qmix_global_tensor(g, x["t0"], r0, x["rows0"], shape) for _, x, g, r0, _ in _views(name)]
    return dict(idq=np.stack(idq), qmix=np.stack(qst))


@functools.lru_cache(maxsize=None)
def idq_reward(name, ints):
    """reward_shaping per view: a tuple of f64 [A] arrays (ints: the ops compared as ints, or as strings)."""
    return tuple(O.idq_reward_shaping(x["t0"], r0, x["t1"], r1, x["op"], ints, x["rows0"], x["A"])
                 for _, x, _, r0, r1 in _views(name))
