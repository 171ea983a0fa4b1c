"""Every step-kernel instantiation the dispatch (select_step, csrc/mdl_kernels.hip) can return,
with the smallest shape that selects it.  Written out by hand from the dispatch rule, like
KERNEL_NAMES in test_gpu_api.py -- not read from the C++ -- so that a kernel added to the
dispatch without an entry here (or an entry the library lost) fails
test_host_cpu.py::test_step_matrix_lists_every_step_kernel, and every entry is stepped against
the CPU oracle by test_gpu_step_matrix.py.

The rule:
  ST    true for the stale ("mappo") tracker, false for the fresh one;
  NCH   package chunks of 64 rounded up to 1, 2, 4, 8, 16 -- P is a class edge (1 | 64, 65 | 128,
        129 | 256, 257 | 512, 513 | 1024), lower and upper alternating inside a class;
  AU    plain and fused steps: up to two chunks 5 for A = 5, 16 for A = 16, 8 for the other A <= 8,
        else 0; from four chunks 8 for A <= 8, else 0 (there A = 5 and A = 16 take the general forms);
        mailbox: 8 for A <= 8, else 0; observations, episode and rows: 5 for A = 5, else 8 (A <= 8);
  NFULL rows: 3 from P = 48, halves (A = 16): 3 from P = 96, else 0.

This module only holds data and the action encoding; it is not a conftest."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# symbol: as rocprof prints it; variant: plain | fused | mail | obs | episode | rows | halves;
# tracker: "mappo" (stale) | "fresh"; subset: a mailbox case that steps env-id subsets
Case = namedtuple("Case", "symbol variant map A P tracker E T seed rng subset",
                  defaults=(5, 25, 42, 0, False))

M1, M3, S64 = "map1.txt", "map3.txt", "synthetic64.txt"   # 64, 100 and far more free cells


def _step(fused):
    v, f = ("fused", "true") if fused else ("plain", "false")

    def c(st, nch, au, mapname, A, P):
        return Case(f"mdl::k_step<{st}, {nch}, {f}, {au}>", v, mapname, A, P, "mappo" if st == "true" else "fresh")
    return c


_p, _f = _step(False), _step(True)


def _m(st, nch, au, mapname, A, P, E=5, subset=False):
    return Case(f"mdl::k_step_mail<{st}, {nch}, {au}>", "mail", mapname, A, P, "mappo" if st == "true" else "fresh",
                E=E, subset=subset)


def _o(kind, st, au, mapname, A, P, seed=42):
    return Case(f"mdl::k_step_{kind}<{st}, {au}>", kind, mapname, A, P, "mappo" if st == "true" else "fresh", seed=seed)


def _r(st, au, nf, mapname, A, P):
    return Case(f"mdl::k_step_rows<{st}, {au}, 4, {nf}>", "rows", mapname, A, P, "mappo" if st == "true" else "fresh", E=6)


def _h(st, nf, mapname, P):
    return Case(f"mdl::k_step_halves<{st}, {nf}>", "halves", mapname, 16, P, "mappo" if st == "true" else "fresh", E=3)


CASES = [
    # ---- k_step<ST, NCH, false, AU>: 28 ----
    _p("true", 1, 5, M1, 5, 1), _p("true", 1, 16, M1, 16, 64), _p("true", 1, 8, M1, 8, 1), _p("true", 1, 0, M1, 9, 64),
    _p("true", 2, 5, M1, 5, 65), _p("true", 2, 16, M3, 16, 128), _p("true", 2, 8, M1, 1, 65), _p("true", 2, 0, M3, 15, 128),
    _p("true", 4, 8, M1, 5, 129), _p("true", 4, 0, M3, 16, 256),
    _p("true", 8, 8, M3, 8, 257), _p("true", 8, 0, M1, 15, 512),
    _p("true", 16, 8, M1, 1, 513), _p("true", 16, 0, S64, 64, 1024),
    _p("false", 1, 5, M3, 5, 64), _p("false", 1, 16, M3, 16, 1), _p("false", 1, 8, M3, 1, 64), _p("false", 1, 0, M3, 17, 1),
    _p("false", 2, 5, M3, 5, 128), _p("false", 2, 16, M1, 16, 65), _p("false", 2, 8, M3, 8, 128), _p("false", 2, 0, M1, 9, 65),
    _p("false", 4, 8, M3, 8, 256), _p("false", 4, 0, M1, 9, 129),
    _p("false", 8, 8, M1, 5, 512), _p("false", 8, 0, M3, 16, 257),
    _p("false", 16, 8, M3, 5, 1024), _p("false", 16, 0, M1, 17, 513),
    # ---- k_step<ST, NCH, true, AU> (mdl_step_fused): 28 ----
    _f("true", 1, 5, M3, 5, 64), _f("true", 1, 16, M3, 16, 1), _f("true", 1, 8, M3, 1, 64), _f("true", 1, 0, M3, 15, 1),
    _f("true", 2, 5, M3, 5, 128), _f("true", 2, 16, M1, 16, 65), _f("true", 2, 8, M3, 8, 128), _f("true", 2, 0, M1, 17, 65),
    _f("true", 4, 8, M3, 1, 256), _f("true", 4, 0, M1, 17, 129),
    _f("true", 8, 8, M1, 5, 512), _f("true", 8, 0, M3, 64, 257),
    _f("true", 16, 8, M3, 8, 1024), _f("true", 16, 0, M1, 16, 513),
    _f("false", 1, 5, M1, 5, 1), _f("false", 1, 16, M1, 16, 64), _f("false", 1, 8, M1, 8, 1), _f("false", 1, 0, M3, 64, 64),
    _f("false", 2, 5, M1, 5, 65), _f("false", 2, 16, M3, 16, 128), _f("false", 2, 8, M1, 1, 65), _f("false", 2, 0, M3, 64, 128),
    _f("false", 4, 8, M1, 5, 129), _f("false", 4, 0, M3, 16, 256),
    _f("false", 8, 8, M3, 1, 257), _f("false", 8, 0, M1, 9, 512),
    _f("false", 16, 8, M1, 5, 513), _f("false", 16, 0, S64, 64, 1024),
    # ---- k_step_mail<ST, NCH, AU> (mdl_mail_step): 20.  E * A > 256 (the action bytes read from the
    # mailbox, not from the kernel arguments): <true, 1, 0>, <false, 2, 0>, <false, 8, 0> ----
    _m("true", 1, 8, M1, 5, 1), _m("true", 1, 0, M3, 64, 64),
    _m("true", 2, 8, M1, 8, 65), _m("true", 2, 0, M3, 16, 128),
    _m("true", 4, 8, M1, 1, 129), _m("true", 4, 0, M3, 9, 256, subset=True),
    _m("true", 8, 8, M1, 5, 257, subset=True), _m("true", 8, 0, M3, 17, 512),
    _m("true", 16, 8, M1, 8, 513), _m("true", 16, 0, M3, 15, 1024),
    _m("false", 1, 8, M3, 8, 64), _m("false", 1, 0, M1, 16, 1),
    _m("false", 2, 8, M3, 5, 128, subset=True), _m("false", 2, 0, M1, 9, 65, E=29),
    _m("false", 4, 8, M3, 8, 256), _m("false", 4, 0, M1, 17, 129),
    _m("false", 8, 8, M3, 1, 512), _m("false", 8, 0, M3, 64, 257),
    _m("false", 16, 8, M3, 5, 1024), _m("false", 16, 0, M1, 9, 513, subset=True),
    # ---- k_step_obs<ST, AU> (mdl_step_obs), k_step_episode<ST, AU> (mdl_step_episode): 4 + 4 (seed 44:
    # with 42 the oracle sees no delivery in either case of that family and tracker mode) ----
    _o("obs", "true", 5, M1, 5, 64), _o("obs", "true", 8, M1, 8, 1),
    _o("obs", "false", 5, M3, 5, 1), _o("obs", "false", 8, M1, 1, 64, seed=44),
    _o("episode", "true", 5, M1, 5, 64, seed=44), _o("episode", "true", 8, M1, 1, 64),
    _o("episode", "false", 5, M1, 5, 1), _o("episode", "false", 8, M1, 8, 64),
    # ---- k_step_rows<ST, AU, 4, NFULL> (step_layout="rows"): 8 ----
    _r("true", 5, 0, M1, 5, 47), _r("true", 5, 3, M1, 5, 64), _r("true", 8, 0, M1, 8, 1), _r("true", 8, 3, M1, 1, 48),
    _r("false", 5, 0, M3, 5, 1), _r("false", 5, 3, M3, 5, 48), _r("false", 8, 0, M3, 1, 47), _r("false", 8, 3, M1, 8, 64),
    # ---- k_step_halves<ST, NFULL> (step_layout="halves", A = 16): 4 ----
    _h("true", 0, M1, 95), _h("true", 3, M3, 128), _h("false", 0, M3, 1), _h("false", 3, M1, 96),
]

SYMBOLS = [c.symbol for c in CASES]

TRAINER_MOVE_CODES = np.array([4, 1, 2, 0, 3], np.uint8)   # as golden_io: D,L,R,S,U -> S=0,L=1,R=2,U=3,D=4


def n_steps(case):
    """Calls per case: two whole episodes of every env and three steps of the third."""
    return 2 * case.T + 3


def trainer_ints(case):
    """The case's actions, uint8 [steps, E, A]: trainer ints 0..14 (MDL_ACTION_TRAINER_INT)."""
    rs = np.random.RandomState(case.rng)
    return rs.randint(0, 15, size=(n_steps(case), case.E, case.A)).astype(np.uint8)


def codes_of(ints):
    """The same actions as MDL_ACTION_CODES bytes: move code | op << 3 (include/mdl_engine.h)."""
    ints = np.asarray(ints, np.uint8)
    return (TRAINER_MOVE_CODES[ints % 5] | ((ints // 5) << 3)).astype(np.uint8)
