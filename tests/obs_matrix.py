"""Every observation-builder instantiation the dispatch (select_obs, csrc/mdl_kernels.hip) can return,
and the cases that run the builders against the CPU oracle at the edges of their run-time layout
decisions.  Written out by hand from the rules -- not read from the C++ -- so that a builder added
to the dispatch without an entry here fails test_host_cpu.py::test_obs_matrix_lists_every_builder_kernel,
and a case whose shape no longer selects its kernel or its path fails test_obs_matrix_cpu.py (the
rule restated in obs_ref.py) and test_gpu_obs_matrix.py (the engine's own obs_kernel_name()).

The rules (csrc/mdl_engine.hip mdl_create, csrc/mdl_obs_small.hpp, csrc/mdl_kernels.hip k_obs):
  ST        true for the stale ("mappo") tracker, false for the fresh one;
  small     obs_builder "auto", A <= 8, P <= 64, the 7-bit-order sort key in 32 bits (key7) and the
            builder's LDS slice for the largest map <= 16,384 B; else the general builder;
  one_pass  small: A*A + A*min(MP, P) + A <= 64 tuple lanes;
  RL        small, several passes, the largest map's rank table <= 8,192 B and table + the launch's
            slices <= 64 KiB: the table is staged in LDS;
  sw        small: MO > A-1 or MP > P (the single-write image; outputs off a 16-B line take the
            early fill instead);
  gen_sort  general: "fast" where the 11-bit-order key fits 32 bits (key32), P <= 64 and A <= 8;
  gen_map   general, by map: "planes" where HW % 4 == 0 and (6A+4)*ceil(maxHW/32) <= 2,048 words,
            "bitrows" for the other HW % 4 == 0 maps, "elem" where HW % 4 != 0.

This module only holds data and the fixture maps; it is not a conftest."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

SYMBOLS = [
    "mdl::k_obs<true>", "mdl::k_obs<false>",
    "mdl::k_obs_h<true, true>", "mdl::k_obs_h<true, false>",
    "mdl::k_obs_h<false, true>", "mdl::k_obs_h<false, false>",
    "mdl::k_obs_small<true, true>", "mdl::k_obs_small<true, false>",
    "mdl::k_obs_small<false, true>", "mdl::k_obs_small<false, false>",
    "mdl::k_obs_small_h<true, true, true>", "mdl::k_obs_small_h<true, true, false>",
    "mdl::k_obs_small_h<true, false, true>", "mdl::k_obs_small_h<true, false, false>",
    "mdl::k_obs_small_h<false, true, true>", "mdl::k_obs_small_h<false, true, false>",
    "mdl::k_obs_small_h<false, false, true>", "mdl::k_obs_small_h<false, false, false>",
]

# facts: small, RL, sw, one_pass (None for the general builder); gen_sort, gen_map (None for the small
# one; gen_map a tuple, one entry per map of the engine).
# steps None: 2T+3 (two auto-resets); points "sixth": every 6th step, the reset step and the one after
# it, the last step; "k32": about eight points around the single reset.
Case = namedtuple("Case", "id maps A P T tracker MO MP MR MPs obsT builder E seed symbol small RL sw one_pass "
                          "gen_sort gen_map steps points env_map")

M0, M1, M2, M3, M4, M5, S64 = ("map.txt", "map1.txt", "map2.txt", "map3.txt", "map4.txt", "map5.txt",
                                "synthetic64.txt")
# fixture maps built here: name -> (H, W, obstacle density, border walls, seed)
BUILT = {"g8x8": (8, 8, 0.10, False, 801), "g5x5": (5, 5, 0.10, False, 501), "g4x8": (4, 8, 0.10, False, 401),
         "r33": (33, 33, 0.15, True, 3301), "r32": (32, 32, 0.15, True, 3201)}


def built_grid(name):
    """A fixture map that is not under marl_gpu/maps: random obstacles from a fixed seed."""
    H, W, dens, border, seed = BUILT[name]
    rs = np.random.RandomState(seed)
    g = (rs.random_sample((H, W)) < dens).astype(np.uint8)
    if border:
        g[0, :] = g[-1, :] = 1
        g[:, 0] = g[:, -1] = 1
    return g


def _c(id, maps, A, P, dims, tracker, symbol, E, T=25, obsT=None, builder="auto", seed=42, small=None, RL=None,
       sw=None, one_pass=None, gen_sort=None, gen_map=None, steps=None, points="sixth", env_map=None):
    maps = (maps,) if isinstance(maps, str) else tuple(maps)
    MO, MP, MR, MPs = dims
    st = {"mappo": "true", "fresh": "false"}[tracker]
    if gen_map is not None and isinstance(gen_map, str):
        gen_map = (gen_map,)
    return Case(id, maps, A, P, T, tracker, MO, MP, MR, MPs, T if obsT is None else obsT, builder, E, seed,
                symbol.format(st=st), small, RL, sw, one_pass, gen_sort, gen_map, steps, points, env_map)


def _s(id, maps, A, P, dims, tracker, E, RL, sw, one_pass, **kw):
    return _c(id, maps, A, P, dims, tracker, "mdl::k_obs_small<{st}, %s>" % ("true" if RL else "false"), E,
              small=True, RL=RL, sw=sw, one_pass=one_pass, **kw)


def _g(id, maps, A, P, dims, tracker, E, gen_sort, gen_map, **kw):
    return _c(id, maps, A, P, dims, tracker, "mdl::k_obs<{st}>", E, small=False, gen_sort=gen_sort, gen_map=gen_map,
              **kw)


D100 = (100, 100, 100, 100)

CASES = [
    # the anchor: config 3's sizes, one pass of 55 lanes
    _s("S1", M1, 5, 50, (4, 5, 100, 100), "mappo", 9, RL=False, sw=False, one_pass=True),
    # the one-pass edge: 64 tuple lanes against 68; 7x7 (HW % 4 != 0); MR < A
    _s("S2a", M0, 4, 20, (3, 11, 3, 10), "fresh", 10, RL=False, sw=False, one_pass=True),
    _s("S2b", M0, 4, 20, (3, 12, 3, 10), "mappo", 11, RL=True, sw=False, one_pass=False),
    # 64 other-robot lanes fill pass one; up to 8 x want package tuples
    _s("S3", M4, 8, 64, (7, 64, 8, 64), "fresh", 13, RL=True, sw=False, one_pass=False),
    # the single-write image; A*Dv = 5035 is odd: rows start at all four g0 % 4; want crosses 6 | 7 with
    # A == 5; MR < A; MPs < nact
    _s("S4", M1, 5, 9, (100, 100, 3, 4), "mappo", 13, RL=True, sw=True, one_pass=False),
    # S4's shape with the padding down to one other-robot slot (MO = 5 > A-1) and MP = 7 < P: with
    # want = 7 an agent's package interval ends where the next agent's begins, so their float4 covers
    # merge (in S4 itself the intervals lie >= 455 floats apart); A*Dv = 335 is odd
    _s("S4m", M1, 5, 9, (5, 7, 3, 4), "fresh", 13, RL=True, sw=True, one_pass=False),
    # sw through MO > A-1 alone; one pass with sw; want crosses 6 | 7 with A != 5; HW = 64: two whole words
    _s("S5", "g8x8", 3, 64, (5, 8, 100, 100), "fresh", 9, RL=False, sw=True, one_pass=True),
    # A = 1, MO = 0, MP > P, want = 0 rows, MR = 1 (no carrier division); HW = 25 < 32.  Fresh: with
    # P <= A + 1 every package starts at t = 0, so a stale tracker could hold no survivor with
    # start_time > t (G3a / G3b likewise: P = 10 < A)
    _s("S6", "g5x5", 1, 2, (0, 5, 1, 5), "fresh", 10, RL=False, sw=True, one_pass=True),
    # MO < A-1 (others cut by rank, ties by index); one package slot; obsT = 50 > T
    _s("S7", M5, 6, 40, (3, 1, 4, 25), "mappo", 11, RL=False, sw=False, one_pass=True, obsT=50),
    # obsT = 0; HW = 32: one whole word and the guard word
    _s("S8", "g4x8", 3, 64, (2, 8, 100, 30), "fresh", 13, RL=False, sw=False, one_pass=True, obsT=0),
    # the small builder on 64x64 (NW = 128: the bitset loops take two trips); LDS slice 15,056 B;
    # several passes, the rank table (32,272 B) stays in global memory
    _s("S9a", S64, 3, 64, (2, 20, 3, 64), "mappo", 9, RL=False, sw=False, one_pass=False),
    _s("S9b", S64, 2, 64, (1, 5, 100, 100), "fresh", 10, RL=False, sw=False, one_pass=True),
    # the same shape through the general builder: plane words exactly 2,048
    _g("S9bg", S64, 2, 64, (1, 5, 100, 100), "mappo", 10, "fast", "planes", builder="generic"),
    # LDS slice 18,128 B > 16,384: the general builder, fast sort, 3,584 plane words -> bit rows
    _g("S9c", S64, 4, 64, (3, 5, 100, 100), "fresh", 9, "fast", "bitrows"),
    # the rank table 8,464 B (off) against 7,952 B (on), both several passes; 33x33 has HW % 4 != 0
    _s("S10a", "r33", 8, 40, (7, 10, 8, 40), "mappo", 9, RL=False, sw=False, one_pass=False),
    _s("S10b", "r32", 8, 40, (7, 10, 8, 40), "fresh", 10, RL=True, sw=False, one_pass=False),
    # the LDS slice exactly 16,384 B (small) against 16,512 B (general); P = 60: 16,256 B, and the table
    # + 4 slices pass 64 KiB (RL off); A = 7, P = 64: 14,960 B (RL on)
    _s("S11a", M4, 8, 61, D100, "fresh", 9, RL=False, sw=True, one_pass=False),
    _g("S11b", M4, 8, 62, D100, "mappo", 10, "fast", "planes"),
    _s("S11c", M4, 8, 60, D100, "mappo", 11, RL=False, sw=True, one_pass=False),
    _s("S11d", M4, 7, 64, D100, "fresh", 13, RL=True, sw=True, one_pass=False),
    # the key7 budget: T = 16182 keeps dl_max < 2^14 (small), 16183 does not (general, and key32 is gone
    # too: the slow sort).  40 steps only, no reset.
    _s("K7a", S64, 3, 64, (2, 20, 3, 64), "fresh", 9, RL=False, sw=False, one_pass=False, T=16182, steps=40),
    _g("K7b", S64, 3, 64, (2, 20, 3, 64), "mappo", 10, "slow", "bitrows", T=16183, steps=40),
    # the key32 budget: T = 822 keeps dl_max < 2^10 (fast sort), 823 does not.  T + 10 steps, one reset.
    _g("K32a", S64, 5, 64, (4, 20, 5, 64), "mappo", 9, "fast", "bitrows", T=822, steps=832, points="k32"),
    _g("K32b", S64, 5, 64, (4, 20, 5, 64), "fresh", 9, "slow", "bitrows", T=823, steps=833, points="k32"),
    # the general builder's fast sort against the oracle directly: S2b's and S4's shapes
    _g("G1a", M0, 4, 20, (3, 12, 3, 10), "fresh", 11, "fast", "elem", builder="generic"),
    _g("G1b", M1, 5, 9, (100, 100, 3, 4), "mappo", 13, "fast", "planes", builder="generic"),
    # A > 8 at P <= 64: the slow sort
    _g("G2", M1, 9, 64, (8, 20, 9, 64), "fresh", 9, "slow", "planes"),
    # plane words 2,002 (planes) against 2,080 (bit rows)
    _g("G3a", M4, 25, 10, (24, 5, 100, 100), "fresh", 9, "slow", "planes"),
    _g("G3b", M4, 26, 10, (24, 5, 100, 100), "fresh", 10, "slow", "bitrows"),
    # per-element maps with the slow sort
    _g("G4", M0, 9, 20, (8, 20, 9, 20), "mappo", 11, "slow", "elem"),
    # two package chunks
    _g("G5", M3, 16, 65, (15, 20, 16, 65), "fresh", 13, "slow", "planes"),
    # one engine over three maps, env groups 3 + 4 + 4: several passes -> RL with the table sized for
    # 20x20, the 7x7 range copies its own table; both builders
    _s("M1", (M0, M2, M3), 4, 20, (3, 12, 3, 10), "mappo", 11, RL=True, sw=False, one_pass=False,
       env_map=(0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2)),
    # two maps of one shape (20x20): the engine's one-launch step + observation kernels take per-env maps
    # (step_obs and step_episode refuse M1's mixed shapes, so this case stands in for M1 there)
    _s("M1s", (M2, M3), 4, 20, (3, 12, 3, 10), "fresh", 11, RL=True, sw=False, one_pass=False,
       env_map=(0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1)),
    _g("M1g", (M0, M2, M3), 4, 20, (3, 12, 3, 10), "fresh", 11, "fast", ("elem", "planes", "planes"),
       builder="generic", env_map=(0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2)),
]

BY_ID = {c.id: c for c in CASES}

# the pairs that straddle an edge: (quantity, lower case, its value, upper case, its value)
EDGES = [
    ("tuple_lanes", "S2a", 64, "S2b", 68),
    ("rank_table_bytes", "S10b", 7952, "S10a", 8464),
    ("small_lds", "S11a", 16384, "S11b", 16512),
    ("key7_T", "K7a", 16182, "K7b", 16183),
    ("key32_T", "K32a", 822, "K32b", 823),
    ("plane_words", "G3a", 2002, "G3b", 2080),
]

# The cases where no compared row has two waiting packages tied on (max(0, dl - t), rank) for an agent (in
# every other case the dict order decides a package order somewhere): recorded from the oracle trace
NO_PKG_TIE = ("K7a", "K7b")

MASKED = ("S1", "S4", "G2", "M1s")   # the cases the masked step_episode test drives


def n_steps(case):
    return 2 * case.T + 3 if case.steps is None else case.steps
