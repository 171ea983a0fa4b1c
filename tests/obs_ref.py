"""The oracle side of tests/obs_matrix.py, the selection rule restated in Python to state each case's
expectations, and the input conditions of test_gpu_obs_matrix.py computed from the oracle alone.

Driving: odd-numbered envs follow OracleGreedy (re-made every episode, as the reference does), so
packages are picked up and delivered and the waiting count reaches 0; the even ones draw uniform
trainer ints.  The greedy (move, op) codes become trainer ints by the inverse of
step_matrix.TRAINER_MOVE_CODES.

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
from golden_io import grid
from obs_matrix import BUILT, built_grid, n_steps
from step_matrix import TRAINER_MOVE_CODES

OBS_KEYS = ("actor_map", "actor_vec", "critic_map", "critic_vec")
ST_WAITING, ST_IN_TRANSIT = 1, 2

_MOVE_TO_INT = np.zeros(5, np.uint8)            # move code -> the trainer move index that decodes to it
_MOVE_TO_INT[TRAINER_MOVE_CODES] = np.arange(5)


def grids(case):
    return [built_grid(m) if m in BUILT else grid(m) for m in case.maps]


def groups(case):
    """[(first env, count, map index)] of the case's runs of envs on one map."""
    em = [0] * case.E if case.env_map is None else list(case.env_map)
    out, b = [], 0
    for e in range(1, case.E + 1):
        if e == case.E or em[e] != em[b]:
            out.append((b, e - b, em[b]))
            b = e
    return out


# ------------------------------------------------------------------ the selection rule, restated
def _bits(v):
    return int(v).bit_length() if v > 0 else 0


@functools.lru_cache(maxsize=None)
def rank_table(H, W):
    """mdl_rank_table (host code of the library): the distance ranks of an H x W map, uint16 [(2H-1)*(2W-1)]."""
    from marl_gpu import _lib
    out = np.zeros((2 * H - 1) * (2 * W - 1), np.uint16)
    assert _lib.lib().mdl_rank_table(H, W, out.ctypes.data) == 0
    return out


def key_budgets(shapes, T):
    """(key7_dsh, key32_dsh): the dlc shift of the 32-bit package sort keys with a 7-bit / 11-bit order
    field, 0 where (order, rank, max(0, dl - t)) does not fit 32 bits; dl_max = T - 1 + 10 + 3H."""
    rank_max = max(int(rank_table(H, W).max()) for H, W in shapes)
    dl_max = max(T - 1 + 10 + 3 * H for H, W in shapes)
    rb, db = _bits(rank_max), _bits(dl_max)
    return (7 + rb if 7 + rb + db <= 32 else 0), (11 + rb if 11 + rb + db <= 32 else 0)


def obs_small_lds(A, HW, P, MO, MP):
    NW = (HW + 31) // 32
    base = (4 * ((6 * A + 9) * NW + 1) + 2 * 256 + 128 + 512 + 64 + 15) & ~15
    MOc, MPc = min(MO, A - 1), min(MP, P)
    if not (MO > MOc or MP > MPc):
        return base
    f4 = A * ((7 + 5 * MOc) // 4 + 2 + (5 * MPc) // 4 + 2) + 2
    return base + 16 * f4 + 16 * 2 * 8 + 16 * 3 * 8


def rank_table_bytes(H, W):
    return ((2 * H - 1) * (2 * W - 1) * 2 + 15) & ~15


def plane_words(A, HW):
    return (6 * A + 4) * ((HW + 31) // 32)


def tuple_lanes(A, P, MP):
    return A * A + A * min(MP, P) + A


def select(case):
    """What the rule gives for the case: dict of symbol (float32) and the path facts of obs_matrix.Case."""
    shapes = [g.shape for g in grids(case)]
    maxHW = max(H * W for H, W in shapes)
    A, P = case.A, case.P
    key7, key32 = key_budgets(shapes, case.T)
    lds = obs_small_lds(A, maxHW, P, case.MO, case.MP)
    small = case.builder == "auto" and 1 <= A <= 8 and 1 <= P <= 64 and key7 > 0 and lds <= 16384
    st = {"mappo": "true", "fresh": "false"}[case.tracker]
    f = dict(small=small, RL=None, sw=None, one_pass=None, gen_sort=None, gen_map=None)
    if small:
        f["one_pass"] = tuple_lanes(A, P, case.MP) <= 64
        f["sw"] = case.MO > min(case.MO, A - 1) or case.MP > min(case.MP, P)
        table = max(rank_table_bytes(H, W) for H, W in shapes) if not f["one_pass"] else 0
        wpb = min(4, 65536 // lds)
        f["RL"] = 0 < table <= 8192 and table + lds * wpb <= 65536
        f["symbol"] = f"mdl::k_obs_small<{st}, {'true' if f['RL'] else 'false'}>"
    else:
        f["gen_sort"] = "fast" if key32 > 0 and P <= 64 and A <= 8 else "slow"
        planes = plane_words(A, maxHW) <= 2048
        f["gen_map"] = tuple("elem" if (H * W) % 4 else "planes" if planes else "bitrows" for H, W in shapes)
        f["symbol"] = f"mdl::k_obs<{st}>"
    return f


def half_symbol(symbol, dtype_name):
    """The float32 symbol's twin for half outputs: k_obs<ST> -> k_obs_h<ST, BF> and so on."""
    bf = "true" if dtype_name == "bfloat16" else "false"
    name, args = symbol[:-1].split("<")
    return f"{name}_h<{args}, {bf}>"


def fused(case):
    """Whether step_obs / step_episode are one launch for the case (the small builder, one map shape)."""
    return bool(case.small) and len({g.shape for g in grids(case)}) == 1


# ------------------------------------------------------------------ the oracle side
def build_points(case):
    """The steps after which the observations are built: every 6th, a reset step (the state is the new
    episode's first) and the one after it, and the last; "k32": about eight around the single reset."""
    n, T = n_steps(case), case.T
    if case.points == "k32":
        pts = {5, T // 2, T - 2, T - 1, T, T + 1, T + 5, n - 1}
    else:
        pts = {k for k in range(n) if k % 6 == 5} | {n - 1}
        for r in range(1, n // T + 1):
            pts |= {r * T - 1, r * T}
    return sorted(k for k in pts if 0 <= k < n)


class Driver:
    """The case's envs: one OracleBatch per map group at seed + the group's first env id (singles: one
    per env at seed + env id -- the same streams -- so that a call can step any subset), the odd envs
    driven by OracleGreedy."""

    def __init__(self, case, singles=False):
        self.case = case
        self.gr = grids(case)
        kw = dict(clear_on_reset=(case.tracker == "fresh"))
        em = [0] * case.E if case.env_map is None else list(case.env_map)
        runs = [(e, 1, em[e]) for e in range(case.E)] if singles else groups(case)
        self.b = [(b0, n, O.OracleBatch(n, self.gr[m], case.A, case.P, case.T, seed_base=case.seed + b0, **kw))
                  for b0, n, m in runs]
        self.rs = np.random.RandomState(case.seed + 1000)
        self.at = {b0 + i: (ob, i) for b0, n, ob in self.b for i in range(n)}
        self.greedy = {e: O.OracleGreedy(self.env(e)) for e in range(1, case.E, 2)}

    def env(self, e):
        ob, i = self.at[e]
        return ob.env(i)

    def tracker(self, e):
        ob, i = self.at[e]
        return ob.tracker(i)

    def actions(self, active=None):
        """Trainer ints [E, A] of the next step (active: only those envs' greedy agents are asked)."""
        c = self.case
        ints = self.rs.randint(0, 15, size=(c.E, c.A)).astype(np.uint8)
        for e, ag in self.greedy.items():
            if active is None or active[e]:
                mv, op = ag.actions(self.env(e))
                ints[e] = _MOVE_TO_INT[mv] + 5 * op
        return ints

    def step(self, ints, auto_reset=True, active=None):
        """One step of every env (active: of the batches whose envs are all set; the others' rows stay
        +0 / not done) -> r, sh, done [E]."""
        c = self.case
        r, sh, dn = np.zeros(c.E, np.float64), np.zeros(c.E, np.float32), np.zeros(c.E, bool)
        for b0, n, ob in self.b:
            if active is not None and not active[b0:b0 + n].any():
                continue
            assert active is None or active[b0:b0 + n].all()
            r[b0:b0 + n], sh[b0:b0 + n], dn[b0:b0 + n] = ob.step(ints[b0:b0 + n], auto_reset=auto_reset,
                                                               consts=O.MAPPO_CONSTS)
        for e in self.greedy:
            if dn[e] and auto_reset:
                self.greedy[e] = O.OracleGreedy(self.env(e))
        return r, sh, dn

    def obs(self):
        """One dict of the four tensors per batch (map group, or env with singles)."""
        c = self.case
        return [ob.obs(c.obsT, c.MO, c.MP, c.MR, c.MPs) for _, _, ob in self.b]

    def rows(self):
        """Every env's (t, robots [A,3] 0-based, tracker rows [n,8], package table [P,8])."""
        out = []
        for e in range(self.case.E):
            st = self.env(e).state()
            out.append((st["t"], st["robots"], self.tracker(e).rows(), st["pkgs"]))
        return out


def walk(case, every_step_obs=False):
    """The case stepped on the oracle: yields (k, ints, (r, sh, done), obs or None, is a build point).
    obs: the list of per-group dicts at the build points (every_step_obs: after every step)."""
    d = Driver(case)
    pts = set(build_points(case))
    for k in range(n_steps(case)):
        ints = d.actions()
        out = d.step(ints)
        yield k, ints, out, (d.obs() if (k in pts or every_step_obs) else None), k in pts


# ------------------------------------------------------------------ the input conditions
def sw_windows(A, Dv, MOc, MO, want, g0):
    """The single-write image's windows for a slab that starts at float g0 (obs_small_emit): the float4
    covers of the 2A+1 data intervals, merged where two share a float4 -> (windows, merges)."""
    S, xe, ps0 = A * Dv, 6 + 5 * MOc, 6 + 5 * MO
    wins, merges = [], 0
    for k in range(2 * A + 1):
        a = k >> 1
        if k == 2 * A:
            s0, s1 = S - 1, S
        elif k & 1:
            s0 = a * Dv + ps0
            s1 = s0 + 5 * want
        else:
            s0, s1 = a * Dv - (1 if a > 0 else 0), a * Dv + xe
        if s1 <= s0:
            continue
        qs, qe = (g0 + s0) >> 2, (g0 + s1 + 3) >> 2
        if wins and qs < wins[-1][1]:
            wins[-1][1] = max(wins[-1][1], qe)
            merges += 1
        else:
            wins.append([qs, qe])
    return wins, merges


@functools.lru_cache(maxsize=None)
def conditions(case):
    """What the compared rows (every env at every build point) hold, from the oracle's trace alone: a
    dict of counts and sets the tests assert on."""
    d = Driver(case)
    gr = d.gr
    em = [0] * case.E if case.env_map is None else list(case.env_map)
    A, P, T = case.A, case.P, case.T
    MOc, MPc = min(case.MO, A - 1), min(case.MP, P)
    Dv = 6 + 5 * case.MO + 5 * case.MP + 1
    pts = set(build_points(case))
    c = dict(rows=0, after_reset=0, carry_tracked=0, survivor_future=0, carry_untracked=0, want=set(),
             want_bins=[0, 0, 0], nact_over=0, g0_mod4=set(), merges=0, other_tie_cut=0, pkg_tie=0, resets=0,
             delivered=0, mr_lt_a=case.MR < A)
    episodes = np.zeros(case.E, np.int64)
    for k in range(n_steps(case)):
        ints = d.actions()
        r, sh, dn = d.step(ints)
        episodes += dn
        c["resets"] += int(dn.sum())
        c["delivered"] += int((r > 0.5).sum())
        if k not in pts:
            continue
        for e, (t, rob, rows, pk) in enumerate(d.rows()):
            H, W = gr[em[e]].shape
            rk = rank_table(H, W)
            c["rows"] += 1
            c["after_reset"] += int(episodes[e] > 0)
            ids = {int(x[0]): x for x in rows}
            carried = [int(x) for x in rob[:, 2] if x != 0]
            c["carry_tracked"] += sum(1 for x in carried if x in ids and ids[x][1] == ST_IN_TRANSIT)
            c["carry_untracked"] += sum(1 for x in carried if not (x in ids and ids[x][1] == ST_IN_TRANSIT))
            # a survivor of an earlier episode: the row differs from the env's package of that id
            for x in rows:
                p = pk[int(x[0]) - 1]
                if tuple(x[2:8]) != tuple(p[0:6]) and x[6] > t:
                    c["survivor_future"] += 1
            wait = [x for x in rows if x[1] == ST_WAITING and x[6] <= t]
            want = min(len(wait), MPc)
            nact = len(wait) + sum(1 for x in rows if x[1] == ST_IN_TRANSIT)
            c["want"].add(want)
            c["want_bins"][0 if want == 0 else 1 if want <= 6 else 2] += 1
            c["nact_over"] += int(nact > case.MPs)
            g0 = e * A * Dv
            c["g0_mod4"].add(g0 % 4)
            if case.sw:
                c["merges"] += int(sw_windows(A, Dv, MOc, case.MO, want, g0)[1] > 0)
            rW, rOff = 2 * W - 1, (H - 1) * (2 * W - 1) + (W - 1)
            for a in range(A):
                oth = sorted((int(rk[rOff + (rob[i, 0] - rob[a, 0]) * rW + (rob[i, 1] - rob[a, 1])]), i)
                             for i in range(A) if i != a)
                if 0 < case.MO < len(oth) and oth[case.MO - 1][0] == oth[case.MO][0]:
                    c["other_tie_cut"] += 1
                keys = [(max(0, int(x[7]) - t) if case.obsT > 0 else 0,
                         int(rk[rOff + (x[2] - rob[a, 0]) * rW + (x[3] - rob[a, 1])])) for x in wait]
                c["pkg_tie"] += int(len(set(keys)) < len(keys))
    return c


def check_inputs(case, c=None):
    """The input conditions of the case (ISSUE: every case, the stale cases, and the named ones)."""
    c = conditions(case) if c is None else c
    cid = case.id
    assert c["rows"] == len(build_points(case)) * case.E
    if not cid.startswith("K7"):
        assert c["after_reset"] > 0 and c["resets"] >= case.E, f"{cid}: no compared row follows an auto-reset"
    assert c["carry_tracked"] > 0, f"{cid}: no compared row has a robot carrying an in-transit tracked package"
    if case.tracker == "mappo" and not cid.startswith("K7"):
        assert c["survivor_future"] > 0, f"{cid}: no survivor of an earlier episode with start_time > t"
        assert c["carry_untracked"] > 0, f"{cid}: no robot carries a package the tracker lacks in transit"
    if cid in ("S4", "S4m", "S5"):
        b = c["want_bins"]
        assert b[0] + b[1] > 0 and b[2] > 0, f"{cid}: want bins {b}"
    if cid in ("S4", "S4m"):
        assert c["g0_mod4"] == {0, 1, 2, 3}, (cid, c["g0_mod4"])
    if cid in ("S4m", "S5"):
        assert c["merges"] > 0, f"{cid}: no row where two intervals' float4 covers merge"
    if cid == "S4":   # its padding keeps every two intervals >= 455 floats apart: S4m carries the merges
        assert c["merges"] == 0
    if case.MPs < case.P and cid in ("S2a", "S2b", "S4", "S4m", "S7", "S8", "G1a", "G1b", "M1", "M1g"):
        assert c["nact_over"] > 0, f"{cid}: no row with nact > MPs"
    if cid in ("S6", "S11b"):   # MPs > P: nact can never pass MPs, every row has zero-filled package rows
        assert case.MPs > case.P and c["nact_over"] == 0
    if cid in ("S2a", "S2b", "S4", "S7"):
        assert c["mr_lt_a"]
    if cid == "S7":
        assert c["other_tie_cut"] > 0, "S7: no rank tie of two other robots across the MO cut"
