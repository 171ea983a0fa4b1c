"""Every per-env launch that draws or consumes a reset -- the seeding, the explicit reset, the tracker
clear, the map-QMIX cycle's lazy reset and the IDQ / qmix builders -- with the shapes that select each
instantiation.  Written out by hand from the dispatch rules (nch_for, launch_reset, launch_cycle_begin,
launch_alt_obs, launch_alt_transition in csrc/mdl_kernels.hip), like step_matrix.py -- not read from
the C++ -- so that a kernel added without an entry here (or an entry the library lost) fails
test_host_cpu.py::test_launch_matrix_lists_every_launch_kernel, and every entry is run against the CPU
oracle by test_gpu_launch_matrix.py.

The rule:
  NCH   package chunks of 64 rounded up to 1, 2, 4, 8, 16 -- P is always a class edge (1 | 64, 65 | 128,
        129 | 256, 257 | 512, 513 | 1024).  k_reset runs both edges of every class with the tracker mode
        alternating, so each NCH sees both modes; k_cycle_begin has one case per symbol, the lower and
        the upper edge alternating so that both edges of every class run across the two modes;
  ST    (k_cycle_begin, k_alt_obs, k_alt_transition) true for the stale ("mappo") tracker, false for
        the fresh one; k_seed, k_reset and k_tracker_clear read the mode from the engine's parameters.
A is spread over 1, 5, 8, 9, 16, 17 and 64, the maps over map.txt (HW = 49: the general emit path of
the builders), map1.txt, map3.txt and synthetic64.txt (A = 64; its P = 1024 cycle case needs about
51 KB of LDS per wavefront, so one wavefront per workgroup).

This module only holds data; it is not a conftest."""
from __future__ import annotations

from collections import namedtuple

# symbol: as rocprof prints it; kind: seed | reset | cycle | alt; tracker: "mappo" (stale) | "fresh";
# mail: the explicit resets go through mail_reset; rounds: steps before each of the three explicit resets (env 1
# is first reset by the second one, at t = T - 1, when every package of its episode has started)
Case = namedtuple("Case", "symbol kind map A P tracker E T seed rng mail rounds",
                  defaults=(6, 25, 42, 0, False, (12, 12, 12)))

M0, M1, M3, S64 = "map.txt", "map1.txt", "map3.txt", "synthetic64.txt"   # 25, 64, 100, 3471 free cells


def _r(nch, mapname, A, P, tracker, **kw):
    return Case(f"mdl::k_reset<{nch}>", "reset", mapname, A, P, tracker, **kw)


def _c(st, nch, mapname, A, P, **kw):
    return Case(f"mdl::k_cycle_begin<{st}, {nch}>", "cycle", mapname, A, P, "mappo" if st == "true" else "fresh",
                **{"E": 5, **kw})


def _a(name, st, mapname, A, P, **kw):
    return Case(f"mdl::{name}<{st}>", "alt", mapname, A, P, "mappo" if st == "true" else "fresh", **{"E": 4, **kw})


CASES = [
    # ---- k_seed: the constructor's draw and the first reset() ----
    Case("mdl::k_seed", "seed", M3, 17, 64, "fresh", E=8),
    # ---- k_reset<NCH>: both edges of every class, each NCH in both modes; two more through mail_reset ----
    _r(1, M0, 1, 1, "fresh"), _r(1, M1, 5, 64, "mappo"),
    _r(2, M3, 8, 65, "mappo"), _r(2, M0, 9, 128, "fresh"),
    _r(4, M1, 16, 129, "fresh"), _r(4, M3, 17, 256, "mappo"),
    _r(8, M0, 5, 257, "mappo"), _r(8, M1, 9, 512, "fresh"),
    _r(16, S64, 64, 513, "fresh", E=4), _r(16, M3, 16, 1024, "mappo", E=4),
    _r(2, M1, 5, 128, "mappo", mail=True), _r(4, M3, 8, 129, "fresh", mail=True),
    # ---- k_tracker_clear: a stale reset case (its third round clears a subset mid-episode) ----
    Case("mdl::k_tracker_clear", "reset", M0, 8, 64, "mappo"),
    # ---- k_cycle_begin<ST, NCH>: one per symbol ----
    _c("false", 1, M0, 1, 1), _c("true", 1, M1, 5, 64),
    _c("false", 2, M3, 8, 128), _c("true", 2, M0, 9, 65),
    _c("false", 4, M1, 16, 129), _c("true", 4, M3, 17, 256),
    _c("false", 8, M0, 5, 512), _c("true", 8, M1, 8, 257),
    _c("false", 16, M3, 9, 513), _c("true", 16, S64, 64, 1024, E=4),
    # ---- k_alt_obs<ST>, k_alt_transition<ST>: every case runs both builders across two auto-resets ----
    _a("k_alt_obs", "true", M1, 5, 64), _a("k_alt_obs", "true", M0, 8, 65),
    _a("k_alt_obs", "false", M0, 5, 64),
    _a("k_alt_transition", "true", M3, 16, 129, E=3), _a("k_alt_transition", "true", S64, 9, 512, E=3),
    _a("k_alt_transition", "false", M1, 17, 128),
]

SYMBOLS = sorted({c.symbol for c in CASES})

# Symbols whose cases are left out because the kernel faulted on the GPU with the cause not found; each
# entry needs a comment naming the fault.  Empty otherwise.
EXCLUDED = set()


def case_id(c):
    return f"{c.symbol}-{c.map.split('.')[0]}-A{c.A}-P{c.P}-{c.tracker}" + ("-mail" if c.mail else "")
