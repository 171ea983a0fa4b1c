"""Helpers of the masked window tests (test_gpu_ego_masked.py, test_ego_masked_cpu.py), on top of ego_ref:
the sentinel bit patterns, the row-mask patterns, the 67-env case that leaves a partial workgroup at every
waves-per-workgroup value, and the episode case -- greedy episodes that end at different steps -- with its
oracle trace.  Everything here is computed from the oracle alone.

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import ego_ref as G
import oracle as O
from golden_io import grid
from obs_ref import _MOVE_TO_INT

# the reused ego_ref cases of the kernel test (the issue's list)
KERNEL_CASES = ("m1_a5_stale", "m1_a5_fresh", "m7_wide_stale", "s64_a16_fresh", "s64_a64_groups", "mixed_stale")

# Sentinels by element size: bit patterns no window element has.  A window holds 0.0 and 1.0 only:
# 0x00000000 / 0x3F800000 as float32, 0x0000 / 0x3C00 as float16, 0x0000 / 0x3F80 as bfloat16.  The float32
# sentinel is a quiet NaN with a payload (compared as bits, never as a float); the 16-bit one differs from
# all three 16-bit values and from both halves of either float32 value, and its two bytes differ, so a
# single written byte shows too.
SENTINEL_BITS = {4: 0x7FC0BEEF, 2: 0x7E5A}
WINDOW_BITS = {"float32": (0x00000000, 0x3F800000), "float16": (0x0000, 0x3C00), "bfloat16": (0x0000, 0x3F80)}


def mask_patterns(E):
    """name -> uint8 [E]: the row masks of the kernel test.  Non-zero means set, whatever the byte."""
    m = {"none": np.zeros(E, np.uint8), "all": np.ones(E, np.uint8)}
    m["first"] = np.zeros(E, np.uint8)
    m["first"][0] = 1
    m["last"] = np.zeros(E, np.uint8)
    m["last"][E - 1] = 1
    m["even"] = (np.arange(E) % 2 == 0).astype(np.uint8)
    m["odd"] = (np.arange(E) % 2 == 1).astype(np.uint8)
    m["bytes"] = np.array([1, 2, 0, 0x80, 0xFF, 0, 0x80, 2], np.uint8)[np.arange(E) % 8]
    return m


# One engine past one workgroup and one XCD round: 67 envs is no multiple of any waves-per-workgroup value
# (1..4) and gives 17 workgroups or more, so the XCD renumbering of the workgroups is live.
BIG = G.Case("m1_a5_e67", (G.M1,), 5, 20, 10, "mappo", (2,), 67, 42, 4, None)


def big_masks():
    E = BIG.E
    but33 = np.ones(E, np.uint8)
    but33[33] = 0
    return {"third": (np.arange(E) % 3 == 0).astype(np.uint8), "but33": but33}


def blocks(E, wpb):
    """(workgroups, waves used in the last one) of a launch over E envs at wpb waves per workgroup."""
    nb = (E + wpb - 1) // wpb
    return nb, E - (nb - 1) * wpb


# The episode case of the step_episode and collector tests: greedy agents on map1 with as many packages as
# robots, so every package is there from t = 0 (P <= A + 1) and the deliveries end episodes early.
Episode = namedtuple("Episode", "map A P T E seed R")
EPISODE = Episode(G.M1, 4, 4, 16, 8, 118, 2)


def codes_to_ints(codes):
    """Engine action codes (move | op << 3) -> the trainer's ints (move index + 5 * op)."""
    codes = np.asarray(codes, np.uint8)
    return (_MOVE_TO_INT[codes & 7] + 5 * (codes >> 3)).astype(np.uint8)


INT_OF_CODE = np.zeros(32, np.uint8)
INT_OF_CODE[[m | (op << 3) for m in range(5) for op in range(3)]] = [
    int(_MOVE_TO_INT[m]) + 5 * op for m in range(5) for op in range(3)]


class EpisodeDriver:
    """One oracle env per engine env (seed + e, fresh tracker), stepped without auto-reset."""

    def __init__(self, ep):
        self.ep = ep
        g = grid(ep.map)
        self.b = [O.OracleBatch(1, g, ep.A, ep.P, ep.T, seed_base=ep.seed + e, clear_on_reset=True)
                  for e in range(ep.E)]

    def step(self, ints, running):
        """Step the envs `running` marks with ints [E, A]; -> done [E] (False where not stepped)."""
        dn = np.zeros(self.ep.E, bool)
        for e in np.nonzero(running)[0]:
            dn[e] = self.b[e].step(ints[e:e + 1], auto_reset=False, consts=O.QMIX_CONSTS)[2][0]
        return dn

    def full(self, e):
        ep = self.ep
        return self.b[e].obs(ep.T, max(ep.A - 1, 0), 5, 4, 4)["actor_map"][0]

    def rows(self, e):
        st = self.b[e].env(0).state()
        return st["t"], st["robots"], self.b[e].tracker(0).rows(), st["pkgs"]


@functools.lru_cache(maxsize=None)
def episode_trace(ep):
    """The episodes under the oracle's greedy agent: dict of ints uint8 [T, E, A], filled bool [T, E] (env e
    took step k), done bool [T, E], length [E], full0 (list of [A, 6, H, W] after the reset) and full
    ([T][E] actor maps after step k, None where the env did not step)."""
    d = EpisodeDriver(ep)
    ag = [O.OracleGreedy(b.env(0)) for b in d.b]
    ints = np.zeros((ep.T, ep.E, ep.A), np.uint8)
    filled = np.zeros((ep.T, ep.E), bool)
    done = np.zeros((ep.T, ep.E), bool)
    full0 = [d.full(e) for e in range(ep.E)]
    full = []
    running = np.ones(ep.E, bool)
    for k in range(ep.T):
        for e in np.nonzero(running)[0]:
            mv, op = ag[e].actions(d.b[e].env(0))
            ints[k, e] = _MOVE_TO_INT[mv] + 5 * op
        filled[k] = running
        done[k] = d.step(ints[k], running)
        full.append([d.full(e) if running[e] else None for e in range(ep.E)])
        running = running & ~done[k]
    return dict(ints=ints, filled=filled, done=done, length=filled.sum(0), full0=full0, full=full)


def episode_conditions(ep):
    """ego_ref's condition counts over the windows the masked builds of the episode case write (radius ep.R):
    every (step, env) with filled set, terminal states included."""
    d = EpisodeDriver(ep)
    tr = episode_trace(ep)
    c = dict.fromkeys(G.CONDITIONS, 0)
    c["windows"] = 0
    R = ep.R
    for k in range(ep.T):
        d.step(tr["ints"][k], tr["filled"][k])
        for e in np.nonzero(tr["filled"][k])[0]:
            full = d.full(e)
            H, W = full.shape[-2:]
            ego = G.ego_from_full(full, R)
            rob = d.rows(e)[1]
            for a in range(ep.A):
                r, cc = (int(v) for v in rob[a, :2])
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
    return c
