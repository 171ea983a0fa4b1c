"""Masked actor-map windows, the checks that need no GPU: the library declares, binds and exports
mdl_build_obs_ego_masked and holds exactly six k_masked_ego_maps instantiations without scratch or SGPR
spill next to the six k_ego_maps; the Python surface; and, on the oracle alone, the input conditions of
test_gpu_ego_masked.py -- episodes that end at different steps, the window conditions the masked builds meet,
sentinels no window element equals, and 67 envs leaving a partial workgroup -- so that the GPU comparison
cannot pass by seeing nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ego_masked_ref as M
import ego_ref as G
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
    m = re.search(r"^int\s+mdl_build_obs_ego_masked\((.*?)\);", txt, re.M | re.S)
    assert m, "mdl_build_obs_ego_masked not declared in mdl_engine.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["MdlEngine* eng", "int32_t env_begin", "int32_t n", "const uint8_t* rows", "int32_t radius",
                    "int32_t dtype", "void* actor_ego", "void* stream"]
    want = ["ptr" if "*" in a else C.c_int32 for a in args]
    res, got = _lib.SIGNATURES["mdl_build_obs_ego_masked"]
    assert res is C.c_int and len(got) == len(want) == 8
    for g, w in zip(got, want):
        assert (g is C.c_void_p) if w == "ptr" else (g is w)
    fn = _lib.lib().mdl_build_obs_ego_masked
    assert list(fn.argtypes) == list(got) and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bT mdl_build_obs_ego_masked\b", out), "mdl_build_obs_ego_masked not exported"
    # the header states the mask's contract
    doc = " ".join(txt[:m.start()].rsplit("/*", 1)[1].split())
    for phrase in ("indexed by ENV ID", "non-zero = build", "rows of unmarked envs are not written",
                   "no host round trip", "hipGraph", "rows == NULL fails"):
        assert phrase in doc, phrase


@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_six_masked_kernels_without_scratch_or_sgpr_spill(tmp_path):
    """k_masked_ego_maps<STALE, OT>, OT in {float, f16_t, bf16_t}: six symbols in the gfx950 code objects,
    none with a private segment or an SGPR spill, within the registers of their unmasked siblings, and none
    that another matrix's name filter (k_ego, k_step, k_obs) would take for one of its own."""
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    masked = sorted(n for n in res if "masked_ego" in n)
    want = sorted(f"_ZN3mdl17k_masked_ego_mapsILb{st}E{ot}EEvNS_9DevParamsEiiiPT0_iiiPKh"
                  for st in (0, 1) for ot in ("f", "NS_5f16_tE", "NS_6bf16_tE"))
    assert masked == want, masked
    for n in masked:
        assert "k_ego" not in n and "k_step" not in n and "k_obs" not in n
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n].get("sgpr_spill_count", 0) == 0, (n, res[n])
        twin = n.replace("17k_masked_ego_maps", "10k_ego_maps").replace("iiiPKh", "iii")
        assert twin in res, twin
        assert res[n]["vgpr_count"] <= res[twin]["vgpr_count"] and res[n]["sgpr_count"] <= res[twin]["sgpr_count"], \
            (res[n], res[twin])


def test_python_surface():
    from marl_gpu.engine import BatchedEnv
    from marl_gpu.evaluate import Evaluator, run_eval
    from marl_gpu.qmix_rollout import QmixCollector
    from marl_gpu.replay import EpisodeReplay
    sig = inspect.signature(BatchedEnv.build_obs_ego_masked).parameters
    assert list(sig)[1:] == ["radius", "rows", "env_begin", "n", "out", "dtype"]
    assert sig["rows"].default is inspect.Parameter.empty   # the unmasked call is build_obs_ego
    assert sig["env_begin"].default == 0 and sig["n"].default is None and sig["out"].default is None
    assert sig["dtype"].default is torch.float32
    doc = " ".join(BatchedEnv.build_obs_ego_masked.__doc__.split())
    assert "indexed by env id" in doc and "not written" in doc and "zeros" in doc
    for fn in (QmixCollector.__init__, Evaluator.__init__, run_eval):
        p = inspect.signature(fn).parameters
        assert p["ego_radius"].default is None and p["ego_dtype"].default is torch.float32, fn
    assert list(inspect.signature(QmixCollector.__init__).parameters)[1:5] == ["env", "episode_limit", "seed", "avail"]
    assert list(inspect.signature(Evaluator.__init__).parameters)[1:3] == ["env", "seed"]
    assert "filled" in QmixCollector.__doc__ and "K, K" in EpisodeReplay.__doc__


def test_sentinels_differ_from_every_window_value():
    """Byte for byte: at every byte position the sentinel differs from both window values of each dtype of
    its size, so a single written byte shows; and the bit patterns are the ones torch holds for 0 and 1."""
    size = {"float32": 4, "float16": 2, "bfloat16": 2}
    for name, vals in M.WINDOW_BITS.items():
        dt = getattr(torch, name)
        es = size[name]
        sent = M.SENTINEL_BITS[es].to_bytes(es, "little")
        for v, x in zip(vals, (0.0, 1.0)):
            vb = v.to_bytes(es, "little")
            assert all(a != b for a, b in zip(sent, vb)), (name, hex(v))
            got = torch.tensor([x], dtype=dt).view({4: torch.int32, 2: torch.int16}[es]).item() & ((1 << 8 * es) - 1)
            assert got == v, (name, x, hex(got))
    assert np.isnan(np.array([M.SENTINEL_BITS[4]], np.uint32).view(np.float32)[0])
    assert len(set(M.SENTINEL_BITS[2].to_bytes(2, "little"))) == 2


def test_mask_patterns():
    for E in (3, 4, 7, 8):
        m = M.mask_patterns(E)
        assert set(m) == {"none", "all", "first", "last", "even", "odd", "bytes"}
        assert not m["none"].any() and m["all"].all()
        assert np.flatnonzero(m["first"]).tolist() == [0] and np.flatnonzero(m["last"]).tolist() == [E - 1]
        assert np.array_equal(m["even"] != 0, ~(m["odd"] != 0)) and m["even"][0] and m["odd"][1]
        assert all(v.dtype == np.uint8 and v.shape == (E,) for v in m.values())
    assert {1, 2, 0x80, 0xFF, 0} == set(M.mask_patterns(8)["bytes"].tolist())
    # the sub-ranges [1, E - 1) and [3, E - 1): a mask read by output row instead of env id marks other rows
    for cid in M.KERNEL_CASES:
        E = G.BY_ID[cid].E
        for b0, n in ((1, E - 2),) + (((3, E - 4),) if E > 4 else ()):
            assert n >= 1
            shifted = [nm for nm, v in M.mask_patterns(E).items()
                       if not np.array_equal(v[b0:b0 + n] != 0, v[:n] != 0)]
            assert shifted, (cid, b0)
    assert [G.BY_ID[c].id for c in M.KERNEL_CASES] == list(M.KERNEL_CASES)
    em = G.BY_ID["mixed_stale"].env_map
    assert len({em[e] for e in range(1, 7)}) == 3   # [1, 7) crosses both map boundaries


def test_67_envs_leave_a_partial_workgroup():
    E = M.BIG.E
    assert E == 67 and M.BIG.A == 5 and M.BIG.P == 20 and M.BIG.radii == (2,)
    for wpb in (1, 2, 3, 4):
        nb, last = M.blocks(E, wpb)
        assert nb > 8, "more workgroups than XCDs: the renumbering permutes them"
        assert wpb == 1 or 0 < last < wpb, (wpb, last)
        assert nb % 8 != 0   # the XCDs hold unequal numbers of workgroups
    masks = M.big_masks()
    assert masks["third"].sum() == 23 and masks["but33"].sum() == 66 and masks["but33"][33] == 0
    assert len(G.build_points(M.BIG)) >= 3 and M.BIG.steps <= 4


def test_episode_case_ends_at_different_steps():
    ep = M.EPISODE
    assert ep.P <= ep.A + 1 and ep.E == 8 and ep.A == 4 and ep.T <= 16
    tr = M.episode_trace(ep)
    L = tr["length"]
    early = L[L < ep.T]
    assert len(early) >= 2 and len(set(early.tolist())) >= 2, L
    assert (L == ep.T).sum() >= 1, L
    assert L.tolist() == [16, 16, 9, 16, 16, 13, 16, 10]
    # every env ends by its own done; `filled` is set up to and including that step, `active` not
    f, d = tr["filled"], tr["done"]
    for e in range(ep.E):
        assert f[:L[e], e].all() and not f[L[e]:, e].any()
        assert d[L[e] - 1, e] and d[:, e].sum() == 1
    # an early end is a delivery of the last package, not the clock
    for e in np.flatnonzero(L < ep.T):
        assert tr["full"][L[e] - 1][e] is not None and tr["full"][min(L[e], ep.T - 1)][e] is None
    # the trainer ints round-trip through the engine's codes
    codes = np.array([m | (op << 3) for m in range(5) for op in range(3)], np.uint8)
    assert sorted(M.codes_to_ints(codes).tolist()) == list(range(15))
    assert np.array_equal(M.INT_OF_CODE[codes], M.codes_to_ints(codes))


def test_episode_case_meets_the_window_conditions():
    """Over the rows the masked builds write (filled == 1, terminal states included) at least one window in
    every condition class the case can reach: all but survivors, which a fresh tracker never holds."""
    ep = M.EPISODE
    got = M.episode_conditions(ep)
    assert got["windows"] == int(M.episode_trace(ep)["filled"].sum()) * ep.A
    for k in sorted(set(G.CONDITIONS) - {"survivor"}):
        assert got[k] > 0, f"no marked window with condition {k!r}"
    assert got["survivor"] == 0
