"""The critic map on a fixed canvas, the checks that need no GPU: the library declares, binds and exports
mdl_build_obs_canvas and holds its twelve kernels without scratch or SGPR spill; the Python surface; the
numpy rule; and, on the oracle alone, the input conditions of test_gpu_canvas.py and
test_gpu_canvas_collect.py -- robots, waiting starts and active targets next to the padding, a tracker
survivor, a package not yet started, a carried package -- so that the GPU comparison cannot pass by seeing
nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import canvas_ref as V
import oracle as O
from test_host_cpu import LLVM_BIN, _kernel_resources

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdl_engine.h")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    O.build()


def test_entry_point_is_declared_bound_and_exported():
    from marl_gpu import _lib
    txt = open(HEADER).read()
    m = re.search(r"^int\s+mdl_build_obs_canvas\((.*?)\);", txt, re.M | re.S)
    assert m, "mdl_build_obs_canvas not declared in mdl_engine.h"
    args = [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in m.group(1).split(",")]
    assert args == ["MdlEngine* eng", "int32_t env_begin", "int32_t n", "const uint8_t* rows", "int32_t dtype",
                    "int32_t canvas_h", "int32_t canvas_w", "void* actor_vec", "void* critic_canvas",
                    "void* critic_vec", "void* stream"]
    want = ["ptr" if "*" in a else C.c_int32 for a in args]
    res, got = _lib.SIGNATURES["mdl_build_obs_canvas"]
    assert res is C.c_int and len(got) == len(want) == 11
    for g, w in zip(got, want):
        assert (g is C.c_void_p) if w == "ptr" else (g is w)
    fn = _lib.lib().mdl_build_obs_canvas
    assert list(fn.argtypes) == list(got) and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT mdl_build_obs_canvas\b", out), "mdl_build_obs_canvas not exported"
    doc = " ".join(txt[:m.start()].rsplit("/*", 1)[1].split())
    for phrase in ("indexed by ENV ID", "non-zero = build", "rows of unmarked envs are not written", "No cropping",
                   "no host round trip", "hipGraph", "may cross map shapes"):
        assert phrase in doc, phrase
    assert _lib.MDL_MAX_CELLS == int(re.search(r"#define MDL_MAX_CELLS (\d+)", txt).group(1))


@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_twelve_kernels_without_scratch_or_sgpr_spill(tmp_path):
    """k_canvas_maps / k_masked_canvas_maps <STALE, OT>, OT in {float, f16_t, bf16_t}: twelve symbols in the
    gfx950 code objects, none with a private segment or an SGPR spill, and none that another matrix's name
    filter (k_ego, k_step, k_obs) would take for one of its own."""
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    got = sorted(n for n in res if "canvas" in n)
    want = sorted([f"_ZN3mdl13k_canvas_mapsILb{st}E{ot}EEvNS_9DevParamsEiiiiPT0_ii"
                   for st in (0, 1) for ot in ("f", "NS_5f16_tE", "NS_6bf16_tE")] +
                  [f"_ZN3mdl20k_masked_canvas_mapsILb{st}E{ot}EEvNS_9DevParamsEiiiiPT0_iiPKh"
                   for st in (0, 1) for ot in ("f", "NS_5f16_tE", "NS_6bf16_tE")])
    assert got == want, got
    for n in got:
        assert "k_ego" not in n and "k_step" not in n and "k_obs" not in n
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n].get("sgpr_spill_count", 0) == 0, (n, res[n])


def test_python_surface():
    from marl_gpu.engine import BatchedEnv
    from marl_gpu.qmix_rollout import QmixCollector
    from marl_gpu.rollout import MappoRollout
    sig = inspect.signature(BatchedEnv.build_obs_canvas).parameters
    assert list(sig)[1:] == ["canvas", "env_begin", "n", "rows", "out", "which", "dtype"]
    assert sig["canvas"].default is inspect.Parameter.empty
    assert sig["env_begin"].default == 0 and sig["n"].default is None and sig["rows"].default is None
    assert sig["out"].default is None and sig["dtype"].default is torch.float32
    assert tuple(sig["which"].default) == ("actor_vec", "critic_map", "critic_vec")
    sig = inspect.signature(BatchedEnv.canvas_buffers).parameters
    assert list(sig)[1:] == ["canvas", "n", "dtype"]
    assert sig["n"].default is None and sig["dtype"].default is torch.float32
    doc = " ".join(BatchedEnv.build_obs_canvas.__doc__.split())
    assert "indexed by env id" in doc and "not written" in doc and "No cropping" in doc
    for cls in (MappoRollout, QmixCollector):
        p = inspect.signature(cls.__init__).parameters
        assert p["canvas"].default is None and list(p)[-1] == "canvas", cls
        assert "canvas" in cls.__doc__ and "ego_radius" in cls.__doc__
    # the parameters before it keep their places
    assert list(inspect.signature(MappoRollout.__init__).parameters)[1:9] == [
        "env", "rollout_steps", "seed", "gamma", "gae_lambda", "avail", "obs_dtype", "ego_radius"]
    assert list(inspect.signature(QmixCollector.__init__).parameters)[1:7] == [
        "env", "episode_limit", "seed", "avail", "ego_radius", "ego_dtype"]
    assert "which=()" in " ".join(BatchedEnv.step_episode.__doc__.split())


def test_canvas_rule():
    rs = np.random.RandomState(3)
    cm = (rs.rand(2, 4, 3, 5) < 0.5).astype(np.float32)
    assert np.array_equal(V.canvas_from_full(cm, 3, 5), cm)   # identity
    c = V.canvas_from_full(cm, 4, 7)
    assert c.shape == (2, 4, 4, 7) and c.dtype == np.float32
    assert np.array_equal(c[..., :3, :5], cm)
    assert (c[:, 0, 3:, :] == 1).all() and (c[:, 0, :, 5:] == 1).all()
    assert (c[:, 1:, 3:, :] == 0).all() and (c[:, 1:, :, 5:] == 0).all()
    with pytest.raises(AssertionError):
        V.canvas_from_full(cm, 3, 4)
    one = V.canvas_from_full(cm[0], 3, 6)   # no leading axis
    assert one.shape == (4, 3, 6) and (one[0, :, 5] == 1).all()


def test_cases_are_the_issues():
    ids = [c.id for c in V.CASES]
    assert len(set(ids)) == len(ids)
    for cid, canvas in (("m1_pad_stale", (12, 13)), ("m1_pad_fresh", (12, 13)), ("m20_id", (20, 20)),
                        ("m20_odd", (21, 23)), ("lines", (9, 12)), ("s64_id", (64, 64)), ("s64_wide", (64, 255)),
                        ("big", (128, 128)), ("mixed_stale", (20, 20)), ("mixed_stale_odd", (21, 23)),
                        ("mixed_fresh", (20, 20)), ("mixed_fresh_odd", (21, 23)), ("e67", (12, 13))):
        assert V.BY_ID[cid].canvas == canvas
    assert {V.BY_ID["m1_pad_stale"].tracker, V.BY_ID["m1_pad_fresh"].tracker} == {"mappo", "fresh"}
    for c in V.CASES:
        Hc, Wc = c.canvas
        assert 1 <= Hc <= 255 and 1 <= Wc <= 255 and Hc * Wc <= 16384
        for H, W in V.shapes(c):
            assert H <= Hc and W <= Wc, c.id
        assert c.steps <= 25 and (c.steps > c.T or c.id == "e67")   # an auto-reset inside the run
    assert V.BY_ID["big"].canvas[0] * V.BY_ID["big"].canvas[1] == 16384
    assert V.BY_ID["s64_wide"].canvas[1] == 255 and V.BY_ID["e67"].E == 67
    assert sorted(set(V.shapes(V.BY_ID["lines"]))) == [(1, 12), (9, 1)]
    for c in V.MIXED:
        sh = V.shapes(c)
        assert sh[0] == (10, 10) and sh[3] == (20, 20) and sh[5] == (7, 7) and c.E == 8
        assert len({sh[e] for e in range(1, c.E - 1)}) == 3   # [1, E - 1) crosses both shape boundaries
    assert len(V.MIXED) == 4
    # odd Hc * Wc with an element count per env that is no multiple of 8: a half-type row 8-B aligned only
    assert (4 * 21 * 23 * 2) % 16 == 8
    # 67 envs: a partial workgroup at every waves-per-workgroup value above one
    for wpb in (2, 3, 4):
        assert 67 % wpb != 0


@pytest.mark.parametrize("cid", ["m1_pad_stale", "lines", "s64_wide", "mixed_stale", "mixed_fresh"])
def test_traces_reset_and_hold_what_the_rule_needs(cid):
    case = V.BY_ID[cid]
    got = V.conditions(V.base(case))
    assert got["resets"] >= case.E, got
    assert got["carried"] > 0, got
    # a waiting entry whose start time lies ahead of the clock is a survivor of an earlier episode: the
    # fresh tracker holds the packages that have appeared, and no other
    if case.tracker == "mappo":
        assert got["survivor"] > 0 and got["not_started"] > 0, got
    else:
        assert got["survivor"] == 0 and got["not_started"] == 0, got


def test_every_condition_is_met_next_to_the_padding():
    """A robot, a waiting start and an active target in a map's last row where the canvas pads below it, and
    in its last column where the canvas pads to the right of it.  map1 and map2 have walls all round, so the
    cases that reach this are the line maps (9 x 12 canvas: the 1 x 12 map's only row is its last, the 9 x 1
    map's only column is its last), the 64 x 255 canvas and the 7 x 7 map of the mixed cases."""
    tot = dict.fromkeys(V.CONDITIONS, 0)
    for cid in ("lines", "s64_wide", "mixed_stale", "mixed_stale_odd"):
        case = V.BY_ID[cid]
        sh = V.shapes(case)
        d = V.Driver(V.base(case))
        pts = set(V.build_points(case))

        def count():
            for e, (H, W) in enumerate(sh):
                cm = d.obs(e)["critic_map"]
                for name, ch in (("robot", 1), ("start", 2), ("target", 3)):
                    if case.canvas[0] > H:
                        tot[name + "_last_row"] += bool(cm[ch, H - 1].any())
                    if case.canvas[1] > W:
                        tot[name + "_last_col"] += bool(cm[ch, :, W - 1].any())
        count()
        for k in range(case.steps):
            d.step(d.actions())
            if k in pts:
                count()
    for k in ("robot_last_row", "robot_last_col", "start_last_row", "start_last_col", "target_last_row",
              "target_last_col"):
        assert tot[k] > 0, (k, tot)


def test_mixed_stale_holds_a_survivor_at_a_build_point():
    got = V.conditions(V.base(V.BY_ID["mixed_stale"]))
    assert got["survivor"] > 0 and got["resets"] >= 8


def test_replay_reproduces_the_driver():
    """The replay driver fed the driver's own actions ends in the driver's state, with and without
    auto-reset."""
    case = V.base(V.BY_ID["mixed_fresh"])
    d, r = V.Driver(case), V.Replay(case)
    for _ in range(12):
        ints = d.actions()
        a, b = d.step(ints), r.step(ints)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for e in range(case.E):
        for k, v in d.obs(e).items():
            assert np.array_equal(v, r.obs(e)[k])
    # without auto-reset only the envs marked running move; a finished env stays where it ended
    q = V.Replay(case, consts=O.QMIX_CONSTS, auto_reset=False)
    running = np.ones(case.E, bool)
    before = q.obs(0)["critic_vec"].copy()
    running[0] = False
    rs = np.random.RandomState(0)
    ended = 0
    for _ in range(case.T):
        _, _, dn = q.step(rs.randint(0, 15, size=(case.E, case.A)), running)
        ended += int(dn.sum())
        running &= ~dn
    assert ended == case.E - 1 and not running.any()
    assert np.array_equal(q.obs(0)["critic_vec"], before)
