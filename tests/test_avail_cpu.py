"""The valid-action mask without a GPU.

The reference has no mask (QMIX/trainer.py:395-397 fills ``avail_u`` with ones), so the rule
(tests/avail_ref.py, include/mdl_engine.h) is pinned against ``env.step`` itself, on the CPU oracle:
a masked action must leave exactly the state its reduction leaves, whatever the other robots do, and
no move, pick-up or delivery that happened may have been masked.  Then the C ABI of the three new
entry points, the register budget of the two new kernels, and ``EpisodeReplay``'s ``avail`` field.

Counts of the four rollouts (seeds and step counts chosen on the oracle; ``test_coverage`` asserts
the conditions, these are the figures at the time of writing):
  small  map.txt 7x7, A=3, P=6,  seed 11, 70 steps:  4 pick-ups, 3 deliveries
  small                          seed 21, 70 steps:  5 pick-ups, 4 deliveries
  map1   map1,       A=5, P=50, seed 3,  90 steps: 10 pick-ups, 5 deliveries
  map1                           seed 21, 90 steps: 10 pick-ups, 5 deliveries
  invalid_move 668, pick_own_only 96, pick_nb_only 181, drop_own 25, drop_nb 66,
  pick_masked_carrying 2819, drop_masked_empty 1793 (robot, move) pairs; 26,768 masked-action probes
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import avail_ref as R  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402
from test_host_cpu import LLVM_BIN, _kernel_resources  # noqa: E402
from test_qmix_cycle_cpu import header_args  # noqa: E402

# T a little above the step count: the packages after the first min(A, 20) + 1 spawn at random
# times below T (env.py:112-116), so a short episode keeps them coming
SHAPES = {"small": dict(mapname="map.txt", A=3, P=6, T=75, steps=70),
          "map1": dict(mapname="map1.txt", A=5, P=50, T=100, steps=90)}
ROLLOUTS = [("small", 11), ("small", 21), ("map1", 3), ("map1", 21)]
P_RANDOM = 0.5       # a robot's greedy action is replaced with this probability
N_JOINT = 8
PROBE_EVERY = 4      # robot i is probed at the steps k with (k + i) % 4 == 0: each probe replays the history
NEW = ("mdl_avail_actions", "mdl_sample_actions_avail", "mdl_sample_actions_avail_dev")


def _env(name, seed):
    c = SHAPES[name]
    o = O.OracleEnv(grid(c["mapname"]), c["A"], c["P"], c["T"], seed=seed)
    o.reset()
    return o


def _raw_step(o, mv, op):
    """``OracleEnv.step`` on prepared uint8 arrays (the replays are the test's cost)."""
    r, ri = C.c_double(), C.c_int()
    d = O.lib().or_env_step(o.h, mv.ctypes.data, op.ctypes.data, C.byref(r), C.byref(ri))
    return r.value, bool(ri.value), bool(d)


def _at(name, seed, history):
    """A fresh env of the shape and seed, brought to the state after ``history`` ([(mv, op)])."""
    o = _env(name, seed)
    for mv, op in history:
        _raw_step(o, mv, op)
    return o


@functools.lru_cache(maxsize=None)
def rollout(name, seed):
    """One history: the oracle's greedy agent, each robot's action replaced with probability
    P_RANDOM by a random one -- half of those uniform over the 15 actions, half uniform over the
    actions the rule leaves available (so pick-ups and drops happen where they can).  Per step: the
    state before it, its mask, and the actions taken (trainer ints); and the state after the last
    step.  Read-only."""
    c = SHAPES[name]
    g = grid(c["mapname"])
    A = c["A"]
    rs = np.random.RandomState(1000 + seed)
    o = _env(name, seed)
    ag = O.OracleGreedy(o)
    inv = np.zeros(5, np.int64)
    inv[[R.MOVE_CODE[m] for m in R.MOVES]] = np.arange(5)     # move code -> trainer move index
    states, masks, acts = [], [], []
    cover = R.new_cover()
    for _ in range(c["steps"]):
        st = o.state()
        mv, op = ag.actions(o)
        a = inv[np.minimum(mv, 4)] + 5 * np.minimum(op.astype(np.int64), 2)
        m = R.mask(g, st["robots"], st["pkgs"], cover)
        u = rs.rand(A)
        for i in range(A):
            if u[i] < P_RANDOM / 2:
                a[i] = rs.randint(0, R.N_ACT)
            elif u[i] < P_RANDOM:
                av = np.nonzero(m[i])[0]
                a[i] = av[rs.randint(0, len(av))]
        states.append(st)
        masks.append(m)
        acts.append(a)
        _, _, done = o.step(*R.codes(a))
        if done:
            break
    states.append(o.state())
    return dict(states=states, masks=masks, acts=acts, cover=cover)


def _same_state(x, y):
    return (x["t"] == y["t"] and x["total_reward"] == y["total_reward"] and np.array_equal(x["robots"], y["robots"])
            and np.array_equal(x["pkgs"], y["pkgs"]))


def _codes(a):
    mv, op = R.codes(a)
    return np.ascontiguousarray(mv, np.uint8), np.ascontiguousarray(op, np.uint8)


@pytest.mark.parametrize("name,seed", ROLLOUTS)
def test_a_masked_action_steps_exactly_as_its_reduction(name, seed):
    ro = rollout(name, seed)
    rs = np.random.RandomState(5)
    A = SHAPES[name]["A"]
    probes = 0
    history = []
    for k, (m, a_hist) in enumerate(zip(ro["masks"], ro["acts"])):
        for i in range(A):
            if (k + i) % PROBE_EVERY:
                continue
            for a in np.nonzero(m[i] == 0)[0]:
                red = R.reduction(int(a), m[i])
                assert m[i, red] == 1 and red != a
                for _ in range(N_JOINT):
                    joint = rs.randint(0, R.N_ACT, A)
                    x, y = _at(name, seed, history), _at(name, seed, history)
                    joint[i] = a
                    rx = _raw_step(x, *_codes(joint))
                    joint[i] = red
                    ry = _raw_step(y, *_codes(joint))
                    assert rx == ry, (name, k, i, int(a), red, rx, ry)
                    assert _same_state(x.state(), y.state()), (name, k, i, int(a), red)
                    probes += 1
        history.append(_codes(a_hist))
    assert probes > 1000
    print(f"{name} seed {seed}: {probes} masked-action probes")


def _events(name, seed):
    """(moved, picked, dropped) bool [steps, A] of the rollout, from consecutive states."""
    ro = rollout(name, seed)
    pre = np.stack([s["robots"] for s in ro["states"][:-1]])
    post = np.stack([s["robots"] for s in ro["states"][1:]])
    moved = (pre[:, :, :2] != post[:, :, :2]).any(-1)
    picked = (pre[:, :, 2] == 0) & (post[:, :, 2] != 0)
    dropped = (pre[:, :, 2] != 0) & (post[:, :, 2] == 0)
    return moved, picked, dropped


@pytest.mark.parametrize("name,seed", ROLLOUTS)
def test_nothing_effective_is_masked(name, seed):
    ro = rollout(name, seed)
    moved, picked, dropped = _events(name, seed)
    m = np.stack(ro["masks"])
    a = np.stack(ro["acts"])
    took_avail = np.take_along_axis(m, a[..., None], -1)[..., 0] == 1
    move_avail = np.take_along_axis(m, (a % 5)[..., None], -1)[..., 0] == 1
    assert move_avail[moved].all() and (a % 5 != R.COL_S)[moved].all()
    assert (a // 5 == 1)[picked].all() and took_avail[picked].all()
    assert (a // 5 == 2)[dropped].all() and took_avail[dropped].all()
    # a carried id never changes into another one within a step
    pre = np.stack([s["robots"][:, 2] for s in ro["states"][:-1]])
    post = np.stack([s["robots"][:, 2] for s in ro["states"][1:]])
    assert ((pre == 0) | (post == 0) | (pre == post)).all()


def test_coverage():
    cover = R.new_cover()
    picks = drops = 0
    for name, seed in ROLLOUTS:
        for k, v in rollout(name, seed)["cover"].items():
            cover[k] += v
        _, picked, dropped = _events(name, seed)
        picks += int(picked.sum())
        drops += int(dropped.sum())
        print(name, seed, len(rollout(name, seed)["acts"]), "steps", int(picked.sum()), "pick-ups",
              int(dropped.sum()), "deliveries")
    print(cover)
    for k in R.COVER:
        assert cover[k] > 0, (k, cover)
    assert picks >= 20 and drops >= 5, (picks, drops)


def test_reduction():
    row = np.zeros(15, np.uint8)
    row[[1, 3, 6, 13]] = 1          # L and S valid; pick-up under L only; drop under S only
    assert R.reduction(3, row) == 3 and R.reduction(6, row) == 6
    assert R.reduction(0, row) == 3          # invalid D -> S
    assert R.reduction(5, row) == 3          # invalid D with pick-up -> S, pick-up unavailable under S -> op 0
    assert R.reduction(10, row) == 13        # invalid D with drop -> S with drop (available under S)
    assert R.reduction(11, row) == 1         # L with drop -> L
    assert R.reduction(8, row) == 3          # S with pick-up -> S


# ---- interface agreement
@pytest.mark.parametrize("name", NEW)
def test_new_entry_points_header_ctypes_and_exports_agree(name):
    from marl_gpu import _lib
    want = header_args(name)
    res, got = _lib.SIGNATURES[name]
    assert res is C.c_int and len(got) == len(want), (name, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if w == "ptr":
            assert g is C.c_void_p or issubclass(g, C._Pointer), f"{name} argument {k}: {g} for a pointer"
        else:
            assert g is w, f"{name} argument {k}: {g} != {w}"
    fn = getattr(_lib.lib(), name)
    assert list(fn.argtypes) == list(got) and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {name}\b", out), f"{name} not exported"


@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_new_kernels_use_no_scratch_and_spill_no_sgpr(tmp_path):
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    for sub in ("k_avail_actions", "k_sample_avail"):
        hit = {k: v for k, v in res.items() if sub in k}
        assert len(hit) == 1, (sub, sorted(hit))
        for k, v in hit.items():
            assert v["private_segment_fixed_size"] == 0, f"{k} uses scratch: {v}"
            assert v.get("sgpr_spill_count", 0) == 0, f"{k} spills SGPRs: {v}"
            assert "k_step" not in k


def test_exports_from_the_package():
    import inspect

    import marl_gpu
    from marl_gpu import actions
    assert hasattr(marl_gpu.BatchedEnv, "avail_actions")
    for fn in (actions.sample_actions, actions.sample_actions_dev):
        assert inspect.signature(fn).parameters["avail"].default is None
    for cls, meth in ((marl_gpu.QmixCollector, "__init__"), (marl_gpu.Evaluator, "run")):
        assert inspect.signature(getattr(cls, meth)).parameters["avail"].default is False
    from marl_gpu.rollout import MappoRollout
    assert inspect.signature(MappoRollout.__init__).parameters["avail"].default is False


# ---- EpisodeReplay on CPU tensors
def _template(L, E, A, with_avail, seed):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.rand(*s, generator=g)                       # noqa: E731
    b = lambda *s: torch.randint(0, 2, s, generator=g, dtype=torch.uint8)   # noqa: E731
    t = dict(so=f(L + 1, E, A, 2, 3, 3), vo=f(L + 1, E, A, 4), gs=f(L + 1, E, 2, 3, 3), gv=f(L + 1, E, 5),
             u=torch.randint(0, 15, (L, E, A), generator=g, dtype=torch.uint8), r=f(L, E), terminated=b(L, E),
             filled=b(L, E))
    if with_avail:
        t["avail"] = b(L + 1, E, A, 15)
    return t


def test_episode_replay_returns_the_stored_masks_shifted_by_one_slot():
    from marl_gpu import EpisodeReplay
    L, E, A = 4, 3, 2
    tpl = _template(L, E, A, True, 0)
    rp = EpisodeReplay(5, tpl)
    assert EpisodeReplay.FIELDS == ("so", "vo", "gs", "gv", "u", "r", "terminated", "filled")
    assert rp.fields == EpisodeReplay.FIELDS + ("avail",)
    rp.add(tpl)
    second = _template(L, E, A, True, 1)
    rp.add(second)                       # wraps: slots 3, 4, 0
    stored = torch.cat((second["avail"][:, 2:], tpl["avail"][:, 1:], second["avail"][:, :2]), 1)   # ring order
    assert torch.equal(rp.buf["avail"], stored)
    s = rp.sample(5, generator=torch.Generator().manual_seed(3))
    idx = torch.randperm(5, generator=torch.Generator().manual_seed(3))[:5]
    want = stored[:, idx].transpose(0, 1).float()
    assert s["avail_u"].dtype == torch.float32 and s["avail_u"].shape == (5, L, A, 15)
    assert torch.equal(s["avail_u"], want[:, :L]) and torch.equal(s["avail_u_next"], want[:, 1:])
    # two views of one gather, as the _next observations are
    assert s["avail_u"].untyped_storage().data_ptr() == s["avail_u_next"].untyped_storage().data_ptr()
    assert torch.equal(s["avail_u"][:, 1:], s["avail_u_next"][:, :-1])


def test_episode_replay_without_the_field_returns_ones():
    from marl_gpu import EpisodeReplay
    L, E, A = 4, 3, 2
    tpl = _template(L, E, A, False, 0)
    rp = EpisodeReplay(4, tpl)
    assert rp.fields == EpisodeReplay.FIELDS and "avail" not in rp.buf
    rp.add(tpl)
    s = rp.sample(2, generator=torch.Generator().manual_seed(3))
    for k in ("avail_u", "avail_u_next"):
        assert s[k].shape == (2, L, A, 15) and s[k].dtype == torch.float32 and bool((s[k] == 1).all())
