"""CPU-oracle side of the evaluation tests (tests/test_eval_cpu.py, tests/test_gpu_eval.py): whole
evaluation episodes -- the greedy agent, or an action tape -- run env by env on the oracle, as
evaluation.py:12-51 runs them, computed once per shape and shared (treat the results as read-only).

The shapes are the ones whose greedy episodes end at many different times, so the device's
running-env mask is exercised: on map1 with seeds 500 + i, i < 24,
  R3  A = 3, P = 3, T = 50   15 episodes end early (shortest 6 steps), 9 run to T; one step kernel
  R9  A = 9, P = 3, T = 50    7 end early (shortest 5 steps), 17 run to T; A > 8: the multi-launch step
"""
import functools

import numpy as np

import oracle as O
from golden_io import grid

E = 24
SEEDS = [500 + i for i in range(E)]
SHAPES = {"R3": dict(mapname="map1.txt", A=3, P=3, T=50), "R9": dict(mapname="map1.txt", A=9, P=3, T=50)}


def final(o):
    """(total_reward, delivered, steps) as evaluation.py:48-50 reads them off a finished env."""
    s = o.state()
    return s["total_reward"], int((s["pkgs"][:, 7] == 3).sum()), s["t"]


@functools.lru_cache(maxsize=None)
def greedy_episodes(name):
    """The 24 greedy episodes of a shape.  Per step k < T: codes[k] uint8 [E, A] (move | op << 3; the
    all-zero row for an env whose episode is over), running[k] bool [E] (the env took step k),
    r[k] f64 [E] and done[k] bool [E] (0 / False for an env that did not step); and the final
    rewards f64 [E], delivered [E], steps [E]."""
    c = SHAPES[name]
    g, A, P, T = grid(c["mapname"]), c["A"], c["P"], c["T"]
    codes = np.zeros((T, E, A), np.uint8)
    running = np.zeros((T, E), bool)
    r = np.zeros((T, E), np.float64)
    done = np.zeros((T, E), bool)
    rewards, delivered, steps = np.zeros(E, np.float64), np.zeros(E, np.int64), np.zeros(E, np.int64)
    for e, seed in enumerate(SEEDS):
        o = O.OracleEnv(g, A, P, T, seed=seed)
        o.reset()
        ag = O.OracleGreedy(o)
        for k in range(T):
            mv, op = ag.actions(o)
            codes[k, e] = np.asarray(mv, np.uint8) | (np.asarray(op, np.uint8) << 3)
            running[k, e] = True
            r[k, e], _, d = o.step(mv, op)
            done[k, e] = d
            if d:
                break
        rewards[e], delivered[e], steps[e] = final(o)
    return dict(codes=codes, running=running, r=r, done=done, rewards=rewards, delivered=delivered, steps=steps)


def tape_episodes(g, A, P, T, seeds, tape, max_steps=None):
    """Episodes driven by an action tape (uint8 [L, E, A], codes): env e, seeded seeds[e], takes
    tape[k, e] at step k until it is done or max_steps steps are taken.  -> rewards, delivered, steps."""
    n = len(seeds)
    L = T if max_steps is None else min(T, max_steps)
    rewards, delivered, steps = np.zeros(n, np.float64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for e, seed in enumerate(seeds):
        o = O.OracleEnv(g, A, P, T, seed=seed)
        o.reset()
        for k in range(L):
            _, _, d = o.step(tape[k, e] & 7, tape[k, e] >> 3)
            if d:
                break
        rewards[e], delivered[e], steps[e] = final(o)
    return rewards, delivered, steps
