"""The map-QMIX cycle (QMixTrainer.collect_and_train_cycle, qmix/trainer.py:329-393) restated on the
CPU oracle, shared by tests/test_qmix_cycle_cpu.py (the oracle side alone) and
tests/test_gpu_qmix_cycle.py (the device side against it).  No GPU here."""
import numpy as np

import oracle as O
from golden_io import grid

TRAINER_MOVE = [O.MOVE_CODES[c] for c in O.TRAINER_MOVES]   # LabelEncoder order D, L, R, S, U

# map, A, P, T, E; forced marks {step: envs}: set in `done` before that step's lazy reset.
# counts: (steps with some but not all envs reset, steps with no reset, resets at t = T, deliveries, pick-ups),
# a delivery being a robot whose carried id goes to 0 in a step and a pick-up one whose carried id leaves 0.
#
# The first three runs are the inputs the feature was specified with.  Stepped with
# RandomState(seed).randint(0, 15) under the trainer's decode, the oracle delivers nothing in any of them
# (every step reward is <= 0: random play rarely delivers within T = 10..14).  Each shape therefore has a
# second run, on the same configuration, steps and marks, whose seed does deliver.
CASES = {
    "map1": dict(cfg=("map1.txt", 5, 20, 12, 9), seed=81, steps=40, marks={3: [1, 4, 6], 17: [0]},
                 counts=(9, 31, 26, 0, 70)),
    "map": dict(cfg=("map.txt", 3, 6, 10, 6), seed=81, steps=36, marks={2: [0, 5], 9: [3]},
                counts=(10, 26, 17, 0, 19)),
    "map2": dict(cfg=("map2.txt", 3, 70, 14, 7), seed=11, steps=40, marks={4: [2, 3]},
                 counts=(5, 35, 14, 0, 30)),
    "map1-delivering": dict(cfg=("map1.txt", 5, 20, 12, 9), seed=13, steps=40, marks={3: [1, 4, 6], 17: [0]},
                            counts=(9, 31, 26, 3, 61)),
    "map-delivering": dict(cfg=("map.txt", 3, 6, 10, 6), seed=68, steps=36, marks={2: [0, 5], 9: [3]},
                           counts=(10, 26, 17, 2, 28)),
    "map2-delivering": dict(cfg=("map2.txt", 3, 70, 14, 7), seed=1, steps=40, marks={4: [2, 3]},
                            counts=(5, 35, 14, 1, 26)),
    # one run per wider package chunking of the lazy reset (P = 129, 257, 513: four, eight, sixteen chunks of
    # 64), which tests/launch_matrix.py covers call by call; counts from the oracle alone, as above
    "map1-nch4": dict(cfg=("map1.txt", 5, 129, 12, 5), seed=81, steps=30, marks={3: [1, 4], 17: [0]},
                      counts=(7, 23, 10, 1, 61)),
    "map-nch8": dict(cfg=("map.txt", 3, 257, 10, 6), seed=81, steps=24, marks={2: [0, 5], 9: [3]},
                     counts=(7, 17, 11, 1, 46)),
    "map3-nch16": dict(cfg=("map3.txt", 3, 513, 12, 5), seed=11, steps=28, marks={4: [2, 3]},
                       counts=(4, 24, 8, 0, 37)),
}
DELIVERING = ("map1-delivering", "map-delivering", "map2-delivering")


def decode(ints):
    """Trainer ints -> (move codes, op codes), qmix/trainer.py:356-362."""
    ints = np.asarray(ints).astype(np.int64)
    op = ints // 5
    return np.array([TRAINER_MOVE[m] for m in ints % 5], np.uint8), np.where(op >= 3, 0, op).astype(np.uint8)


def features(g, env, trk, A, state_shape):
    t, r1, rows = env.state()["t"], env.robots1(), trk.rows()
    return (np.stack([O.idq_convert_state(g, t, r1, rows, a) for a in range(A)]),
            O.qmix_global_tensor(g, t, r1, rows, state_shape))


def oracle_cycle(case, state_shape=None):
    """Yields one record per time step: the actions, the envs the lazy reset took (``marked``), their
    banked return and length, the observations / state before and after the step, the global
    reward, done, and the step's deliveries and pick-ups."""
    mapname, A, P, T, E = case["cfg"]
    g = grid(mapname)
    H, W = g.shape
    shape = (7, H, W) if state_shape is None else tuple(state_shape)
    ob = O.OracleBatch(E, g, A, P, T, seed_base=case["seed"], clear_on_reset=True)   # the constructor: reset + update
    rs = np.random.RandomState(case["seed"])
    done = np.zeros(E, bool)
    for k in range(case["steps"]):
        for e in case["marks"].get(k, ()):
            done[e] = True
        ints = rs.randint(0, 15, size=(E, A)).astype(np.uint8)
        rec = dict(k=k, ints=ints, marked=done.copy(), completed_return=np.zeros(E, np.float64),
                   completed_steps=np.zeros(E, np.int32), obs=np.zeros((E, A, 6, H, W), np.float32),
                   state=np.zeros((E,) + shape, np.float32), next_obs=np.zeros((E, A, 6, H, W), np.float32),
                   next_state=np.zeros((E,) + shape, np.float32), r_env=np.zeros(E, np.float64),
                   deliveries=0, pickups=0, resets_at_T=0)
        for e in range(E):
            env, trk = ob.env(e), ob.tracker(e)
            if done[e]:                                   # qmix/trainer.py:331-341
                st = env.state()
                rec["completed_return"][e] = st["total_reward"]
                rec["completed_steps"][e] = st["t"]
                rec["resets_at_T"] += int(st["t"] == T)
                env.reset()
                trk.clear()
                trk.update_from_env(env)
                done[e] = False
            rec["obs"][e], rec["state"][e] = features(g, env, trk, A, shape)
            pc = env.robots1()[:, 2].copy()
            mv, op = decode(ints[e])
            r, _, d = env.step(mv, op)
            trk.update_from_env(env)
            rec["next_obs"][e], rec["next_state"][e] = features(g, env, trk, A, shape)
            cc = env.robots1()[:, 2]
            rec["pickups"] += int(((pc == 0) & (cc != 0)).sum())
            rec["deliveries"] += int(((pc != 0) & (cc == 0)).sum())
            rec["r_env"][e] = r
            done[e] = d
        rec["done"] = done.copy()
        yield rec


def counts(records, E):
    n = [int(r["marked"].sum()) for r in records]
    return (sum(1 for x in n if 0 < x < E), sum(1 for x in n if x == 0), sum(r["resets_at_T"] for r in records),
            sum(r["deliveries"] for r in records), sum(r["pickups"] for r in records))




class NumpyJointRing:
    """What the qmix/ trainer's joint replay buffer holds after its one-row-at-a-time adds, written as
    a ring of named numpy arrays: the row of env e of a time step lands in slot (ptr + e) % capacity,
    envs in order (a later env overwrites an earlier one where a step is larger than the ring)."""

    FIELDS = ("states", "next_states", "observations", "next_observations", "actions", "total_reward", "dones")

    def __init__(self, capacity, A, obs_shape, state_shape):
        self.capacity, self.ptr, self.size = capacity, 0, 0
        tail = dict(states=state_shape, next_states=state_shape, observations=(A,) + obs_shape,
                    next_observations=(A,) + obs_shape, actions=(A,), total_reward=(1,), dones=(1,))
        kind = dict(actions=np.int64, dones=np.bool_)
        for name in self.FIELDS:
            setattr(self, name, np.zeros((capacity,) + tail[name], kind.get(name, np.float32)))

    def add_step(self, state, next_state, obs, next_obs, actions, reward, done):
        """One time step: every env adds its row, in env order."""
        step = dict(states=state, next_states=next_state, observations=obs, next_observations=next_obs,
                    actions=actions, total_reward=np.asarray(reward).reshape(-1, 1),
                    dones=np.asarray(done).astype(bool).reshape(-1, 1))
        E = actions.shape[0]
        for e in range(E):
            slot = (self.ptr + e) % self.capacity
            for name in self.FIELDS:
                getattr(self, name)[slot] = step[name][e]
        self.ptr = (self.ptr + E) % self.capacity
        self.size = min(self.size + E, self.capacity)
