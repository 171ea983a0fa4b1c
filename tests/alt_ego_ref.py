"""The reference rule of the robot-centred IDQ / map-QMIX windows (BatchedEnv.build_obs_alt_ego), the
cases of test_gpu_alt_ego.py and their input conditions, computed from the oracle alone.

The rule: the window is a crop of the reference's own convert_state tensor (oracle.idq_convert_state)
around the robot's cell (the single 1 of channel 4), padded with ones in channel 0 and zeros in channels
1-5.  Channel 1 holds float32 urgencies, so every comparison downstream is on bit patterns.

The cases reuse ego_ref.Case and its driver: odd-numbered envs follow OracleGreedy (re-made every
episode), so packages are picked up and carried; the even ones draw uniform trainer ints; auto-reset;
one OracleBatch per env at seed + env id, the engine's own seeds.

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import functools

import numpy as np

import ego_ref as G
import oracle as O

ST_WAITING = 1


def alt_ego_from_full(full, R):
    """full [.., A, 6, H, W] (idq_convert_state per agent) -> [.., A, 6, K, K], K = 2R + 1."""
    full = np.asarray(full)
    H, W = full.shape[-2:]
    K = 2 * R + 1
    flat = full.reshape(-1, 6, H, W)
    pad = np.zeros((flat.shape[0], 6, H + 2 * R, W + 2 * R), full.dtype)
    pad[:, 0] = 1
    pad[:, :, R:R + H, R:R + W] = flat
    out = np.empty((flat.shape[0], 6, K, K), full.dtype)
    for k in range(flat.shape[0]):
        pos = np.argwhere(flat[k, 4] == 1)
        assert len(pos) == 1, "channel 4 holds the robot's cell alone"
        r, c = pos[0]
        out[k] = pad[k, :, r:r + K, c:c + K]
    return out.reshape(full.shape[:-2] + (K, K))


M0, M1, M2, S64 = G.M0, G.M1, G.M2, G.S64
_c = G._c

# The issue's list.  Seeds were re-drawn until every case meets test_alt_ego_cpu.py's input conditions.
CASES = [
    # odd A: an env row is 24 * 5 * K^2 bytes, every second one only 8-B aligned
    _c("m1_a5_stale", M1, 5, 20, 10, "mappo", (1, 2), 8),
    _c("m1_a5_fresh", M1, 5, 20, 18, "fresh", (1, 2), 7, seed=45),
    # the window wider than the map; one-row and one-column maps
    _c("m7_wide_stale", M0, 4, 12, 10, "mappo", (5, 15), 8),
    _c("m7_wide_fresh", M0, 4, 12, 16, "fresh", (5, 15), 5),
    _c("line1x12", "line1x12", 3, 6, 13, "mappo", (2,), 8),
    _c("line9x1", "line9x1", 2, 5, 16, "fresh", (2,), 8),
    # 20x20: map rows start in mid-word
    _c("m20_a8_stale", M2, 8, 30, 10, "mappo", (3,), 8),
    _c("m20_a8_fresh", M2, 8, 30, 24, "fresh", (3,), 6),
    # 64x64: two words per map row, windows across column 32
    _c("s64_a16_stale", S64, 16, 100, 12, "mappo", (5, 15), 8),
    _c("s64_a16_fresh", S64, 16, 100, 12, "fresh", (5, 15), 4, seed=43),
    # the robot groups (A = 64, R = 15: the image of all robots is 46 KB)
    _c("s64_a64_groups", S64, 64, 100, 12, "mappo", (15,), 3),
    # one engine over three map shapes; the tests also build one range across both boundaries
    _c("mixed_stale", (M1, M2, M0), 4, 12, 10, "mappo", (2, 5), 8, env_map=(0, 0, 0, 1, 1, 2, 2, 2)),
    _c("mixed_fresh", (M1, M2, M0), 4, 12, 18, "fresh", (3,), 7, env_map=(0, 0, 1, 1, 1, 2, 2)),
]
BY_ID = {c.id: c for c in CASES}
SINGLE_MAP = tuple(c.id for c in CASES if len(c.maps) == 1)

build_points = G.build_points


class Driver(G.Driver):
    """ego_ref's driver with the IDQ featurizer's tensors."""

    def full(self):
        """The oracle's convert_state of every agent of every env: a list of [A, 6, H, W]."""
        c = self.case
        em = G.env_maps(c)
        out = []
        for e, ob in enumerate(self.b):
            env = ob.env(0)
            t, r1, rows = env.state()["t"], env.robots1(), ob.tracker(0).rows()
            out.append(np.stack([O.idq_convert_state(self.gr[em[e]], t, r1, rows, a) for a in range(c.A)]))
        return out


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


def urgency(t, st, dl):
    """convert_state's urgency of a waiting, started package (IDQ/networks.py:150-160), as a float."""
    if dl > st:
        return min(1.0, max(0.0, (t - st) / (dl - st)))
    return 1.0 if dl == st else 0.0


CONDITIONS = ("top", "bottom", "left", "right", "corner", "other", "frac", "one", "max_rule", "carry_hidden",
              "carried_in", "carried_out", "survivor")


@functools.lru_cache(maxsize=None)
def conditions(case, R):
    """How many windows of the case's build points (radius R) meet each input condition; also
    "unaligned_ch1": non-zero channel-1 elements in env rows that start off a 16-byte line when the
    output of the whole engine starts on one."""
    d = Driver(case)
    pts = set(build_points(case))
    c = dict.fromkeys(CONDITIONS, 0)
    c["resets"] = c["windows"] = c["unaligned_ch1"] = 0
    K = 2 * R + 1

    def count():
        for e, full in enumerate(d.full()):
            H, W = full.shape[-2:]
            ego = alt_ego_from_full(full, R)
            t, rob, rows, pk = d.rows(e)
            waiting = [x for x in rows if x[1] == ST_WAITING and x[6] <= t]
            by_cell = {}
            for x in waiting:
                by_cell.setdefault((int(x[2]), int(x[3])), set()).add(urgency(t, int(x[6]), int(x[7])))
            multi = [cell for cell, us in by_cell.items() if len(us) > 1]
            surv = [(int(x[2]), int(x[3])) for x in waiting if tuple(x[2:8]) != tuple(pk[int(x[0]) - 1][0:6])]
            shows = [a for a in range(case.A) if rob[a, 2] == 0 and ego[a, 2].any()]
            if (e * case.A * 6 * K * K) % 4:
                c["unaligned_ch1"] += int(np.count_nonzero(ego[:, 1]))
            for a in range(case.A):
                r, cc = (int(v) for v in rob[a, :2])
                assert full[a, 4, r, cc] == 1 and ego[a, 4, R, R] == 1 and ego[a, 4].sum() == 1
                inside = lambda cell: abs(cell[0] - r) <= R and abs(cell[1] - cc) <= R  # noqa: E731
                top, bottom, left, right = r - R < 0, r + R >= H, cc - R < 0, cc + R >= W
                free = rob[a, 2] == 0
                c["windows"] += 1
                c["top"] += top
                c["bottom"] += bottom
                c["left"] += left
                c["right"] += right
                c["corner"] += (top or bottom) and (left or right)
                c["other"] += bool(ego[a, 3].any())
                c["frac"] += bool(((ego[a, 1] > 0) & (ego[a, 1] < 1)).any())
                c["one"] += bool((ego[a, 1] == 1).any())
                c["max_rule"] += bool(free and any(inside(cell) for cell in multi))
                if not free:
                    assert not ego[a, 1].any() and not ego[a, 2].any()
                    c["carry_hidden"] += bool(any(inside(cell) for cell in by_cell) and
                                              any(b != a for b in shows))
                c["carried_in"] += bool(ego[a, 5].any())
                c["carried_out"] += bool(not free and full[a, 5].any() and not ego[a, 5].any())
                c["survivor"] += bool(free and any(inside(cell) for cell in surv))

    count()
    for k in range(case.steps):
        c["resets"] += int(d.step(d.actions()).sum())
        if k in pts:
            count()
    return c


def expected(case, R):
    """The conditions the case must meet at radius R: all of them, less what its maps rule out
    (ego_ref.expected's rules for the sides and the carried target outside the window) and survivors
    with the fresh tracker."""
    want = set(CONDITIONS)
    keep = G.expected(case, R)
    for k in ("top", "bottom", "left", "right", "corner", "carried_out"):
        if k not in keep:
            want.discard(k)
    if case.tracker != "mappo":
        want.discard("survivor")
    # an urgency of exactly 1.0 needs t >= deadline: a package's deadline is 10 + randint(H // 2, 3 * H) past
    # its start (env.py's generator, H the map's row count) and an episode shows t <= T - 1
    if not any(10 + g.shape[0] // 2 <= case.T - 1 for g in G.grids(case)):
        want.discard("one")
    return want
