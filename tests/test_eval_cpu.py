"""The device-resident evaluation without a GPU: the C ABI of the two new entry points (header,
ctypes signatures and the built library's exports agree); the register budget of their kernels
from the code objects' metadata; the random agent's action tape and ``summary()``'s arithmetic
against the reference's recorded evaluation (tests/golden/eval_anchor.json); and the counts that
keep the oracle's greedy episodes, which tests/test_gpu_eval.py compares the device against, from
being a quiet run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eval_ref as R  # noqa: E402
from golden_io import grid, load_json  # noqa: E402
from test_host_cpu import LLVM_BIN, _kernel_resources  # noqa: E402
from test_qmix_cycle_cpu import header_args  # noqa: E402

NEW = ("mdl_greedy_actions_masked", "mdl_episode_results")


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
    L = _lib.lib()
    fn = getattr(L, name)
    assert list(fn.argtypes) == list(got) and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {name}\b", out), f"{name} not exported"


@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_new_kernels_use_no_scratch_and_spill_no_sgpr(tmp_path):
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    results = {k: v for k, v in res.items() if "k_episode_results" in k}
    act = {k: v for k, v in res.items() if "k_greedy_act" in k}
    assert len(results) == 1, sorted(results)
    assert len(act) == 1, sorted(act)             # one kernel with a nullable mask, no sibling
    for k, v in {**results, **act}.items():
        assert v["private_segment_fixed_size"] == 0, f"{k} uses scratch: {v}"
        assert v.get("sgpr_spill_count", 0) == 0, f"{k} spills SGPRs: {v}"
        assert "k_step" not in k


def test_exports_from_the_package():
    import marl_gpu
    from marl_gpu import evaluate
    assert marl_gpu.Evaluator is evaluate.Evaluator and marl_gpu.run_eval is evaluate.run_eval
    assert marl_gpu.random_action_tape is evaluate.random_action_tape
    assert hasattr(marl_gpu.BatchedEnv, "greedy_actions_masked") and hasattr(marl_gpu.BatchedEnv, "episode_results")


# ---- the random agent's tape reproduces the reference's recorded random episodes
def test_random_action_tape_reproduces_the_anchor_on_the_oracle():
    from marl_gpu.evaluate import random_action_tape
    ref = load_json("eval_anchor.json")
    cfg = ref["config"]
    A, P, T = cfg["n_agents"], cfg["n_packages"], cfg["max_time_steps"]
    tape = random_action_tape(cfg["seed"], 3, A, T)
    assert tape.shape == (T, 3, A) and tape.dtype == np.uint8
    assert int((tape & 7).max()) <= 4 and int((tape >> 3).max()) <= 2
    rewards, delivered, steps = R.tape_episodes(grid(cfg["map"]), A, P, T, [cfg["seed"] + ep for ep in range(3)], tape)
    assert steps.tolist() == [T] * 3
    assert rewards.tolist() == ref["random"]["rewards"][:3] == [-4.009999999999955, -22.079999999999863,
                                                                 -14.76999999999969]
    assert delivered.tolist() == ref["random"]["delivered"][:3] == [21, 11, 18]


def test_random_action_tape_is_the_choice_stream():
    """The tape's draws are ``np.random.choice``'s: the literal randomagent.py loop under
    ``np.random.seed`` on a small case, episode-major."""
    from marl_gpu.evaluate import random_action_tape
    code = {"S": 0, "L": 1, "R": 2, "U": 3, "D": 4}
    state = np.random.get_state()
    try:
        np.random.seed(77)
        want = np.zeros((4, 2, 3), np.uint8)
        for ep in range(2):
            for k in range(4):
                for a in range(3):
                    move = np.random.choice(['U', 'D', 'L', 'R', 'S'])
                    act = np.random.choice(['0', '1', '2'])
                    want[k, ep, a] = code[str(move)] | (int(act) << 3)
    finally:
        np.random.set_state(state)
    assert np.array_equal(random_action_tape(77, 2, 3, 4), want)


# ---- summary()'s arithmetic is the reference's
@pytest.mark.parametrize("agent", ["greedy", "random"])
def test_summarize_reproduces_the_anchor_statistics(agent):
    from marl_gpu.evaluate import summarize
    ref = load_json("eval_anchor.json")
    rec = ref[agent]
    s = summarize(rec["rewards"], rec["delivered"], ref["config"]["n_packages"])
    assert s["rewards"] == rec["rewards"] and s["delivered"] == rec["delivered"]
    for k in ("mean_reward", "std_reward", "mean_delivered", "std_delivered"):
        assert float(s[k]) == rec[k], (k, float(s[k]), rec[k])
    P = ref["config"]["n_packages"]
    assert s["delivery_rate"] == [(d / P) * 100 for d in rec["delivered"]]
    assert float(s["mean_delivery_rate"]) == float(np.mean(s["delivery_rate"]))
    assert float(s["std_delivery_rate"]) == float(np.std(s["delivery_rate"]))
    empty = summarize([], [], P)
    assert empty["rewards"] == [] and empty["mean_reward"] == 0 and empty["std_delivered"] == 0


# ---- the oracle's greedy episodes: not a quiet run
@pytest.mark.parametrize("name,early,full", [("R3", 15, 9), ("R9", 7, 17)])
def test_oracle_greedy_episodes_end_at_many_times(name, early, full):
    ep = R.greedy_episodes(name)
    T = R.SHAPES[name]["T"]
    steps = ep["steps"]
    n_early, n_full = int((steps < T).sum()), int((steps == T).sum())
    assert n_early >= 5 and n_full >= 5
    assert (n_early, n_full) == (early, full)
    assert np.array_equal(ep["running"].sum(0), steps)
    assert np.array_equal(ep["done"].sum(0), np.ones(R.E, np.int64))          # every episode ends once
    assert not ep["codes"][~ep["running"]].any()
