"""The valid-action rule (include/mdl_engine.h, ``mdl_avail_actions``) in plain numpy, for
tests/test_avail_cpu.py and tests/test_gpu_avail.py: the mask of one env from the tables that
``read_state`` / ``OracleEnv.state`` export (robots [A, 3] = r, c, carry; pkgs [P, 8] = sr, sc, tr, tc,
start_time, deadline, id, status) and the map grid, the reduction of a masked action, and the
counters of the situations the tests must have met.

Columns are the trainer-int order: column a = move 'D','L','R','S','U'[a % 5], op a // 5.
"""
import numpy as np

N_ACT = 15
MOVES = "DLRSU"
DELTA = {"S": (0, 0), "L": (0, -1), "R": (0, 1), "U": (-1, 0), "D": (1, 0)}
MOVE_CODE = {"S": 0, "L": 1, "R": 2, "U": 3, "D": 4}
ST_WAITING = 1
COL_S = MOVES.index("S")          # column of ('S', op 0)

# what a run must have met (test_*: "coverage is a condition")
COVER = ("invalid_move", "pick_own_only", "pick_nb_only", "drop_own", "drop_nb", "pick_masked_carrying",
         "drop_masked_empty")


def valid_position(grid, r, c):
    H, W = grid.shape
    return 0 <= r < H and 0 <= c < W and grid[r, c] == 0


def mask(grid, robots, pkgs, cover=None):
    """uint8 [A, 15] of one env.  cover: a dict of counters (COVER's names) to add to."""
    A = robots.shape[0]
    out = np.zeros((A, N_ACT), np.uint8)
    waiting = {(int(p[0]), int(p[1])) for p in pkgs if p[7] == ST_WAITING}
    for i in range(A):
        r, c, carry = (int(x) for x in robots[i])
        target = None
        if carry:
            p = pkgs[carry - 1]
            target = (int(p[2]), int(p[3]))
        for mi, m in enumerate(MOVES):
            dr, dc = DELTA[m]
            prop = (r + dr, c + dc)
            if m != "S" and not valid_position(grid, *prop):
                if cover is not None:
                    cover["invalid_move"] += 1
                continue
            out[i, mi] = 1
            own, nb = (r, c), prop
            if carry == 0:
                p_own, p_nb = own in waiting, nb in waiting
                out[i, 5 + mi] = p_own or p_nb
                if cover is not None and m != "S":
                    cover["pick_own_only"] += p_own and not p_nb
                    cover["pick_nb_only"] += p_nb and not p_own
                    cover["drop_masked_empty"] += 1
            else:
                out[i, 10 + mi] = target == own or target == nb
                if cover is not None and m != "S":
                    cover["drop_own"] += target == own
                    cover["drop_nb"] += target == nb
                    cover["pick_masked_carrying"] += 1
    return out


def masks(grids, robots, pkgs, cover=None):
    """uint8 [E, A, 15] from the batched tables; grids: one grid or one per env."""
    E = robots.shape[0]
    per_env = isinstance(grids, (list, tuple))
    return np.stack([mask(grids[e] if per_env else grids, robots[e], pkgs[e], cover) for e in range(E)])


def reduction(a, mask_row):
    """The action an unavailable action ``a`` is certain to equal: an invalid move becomes 'S', then
    an op unavailable under the resulting move becomes 0.  An available action is its own reduction."""
    mi, op = a % 5, a // 5
    if not mask_row[mi]:
        mi = COL_S
    if not mask_row[5 * op + mi]:
        op = 0
    return 5 * op + mi


def codes(a):
    """(move code, op code) of trainer-int action(s) ``a``, as ``OracleEnv.step`` takes them."""
    a = np.asarray(a)
    mv = np.array([MOVE_CODE[m] for m in MOVES], np.uint8)[a % 5]
    return mv, (a // 5).astype(np.uint8)


def new_cover():
    return {k: 0 for k in COVER}
