"""Half-precision observations, the checks that need no GPU: the reference conversion
(obs_dtype_ref.round_to) agrees with numpy's on the oracle's observations; the rounding-edge inputs of
test_gpu_obs_dtype.py really are edges (a bf16 tie, an fp16 tie, an inexact fp16 subnormal), on the
oracle alone; the library holds the half instantiations of both builders without scratch and no other
new step or launch-matrix kernel; the new entry points are declared, bound and exported."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import oracle as O
from golden_io import grid
from obs_dtype_ref import HALF_DTYPES, OBS_KEYS, has_fp16_subnormal, has_tie, round_to
from test_host_cpu import LAUNCH_KERNELS, LLVM_BIN, _kernel_resources, _launch_mangled_prefix, _mangled_prefix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdl_engine.h")
NEW = ("mdl_build_obs_as", "mdl_step_obs_as")


def test_reference_conversion_is_numpys_on_oracle_observations():
    """torch's CPU float32 -> float16 conversion (the reference of every half test) and numpy's astype
    give the same bits on the observations of a short MAPPO rollout; bf16 (numpy has none) is checked
    against round-to-nearest-even written out on the bit pattern."""
    g = grid("map1.txt")
    E, A, P, T = 4, 5, 50, 40
    ob = O.OracleBatch(E, g, A, P, T, seed_base=42, clear_on_reset=False)
    gen = np.random.RandomState(3)
    seen_inexact = False
    for k in range(50):   # across the auto-reset at t = T
        ob.step(gen.randint(0, 15, size=(E, A)).astype(np.uint8), auto_reset=True, consts=O.MAPPO_CONSTS)
        if k % 7 == 3:
            obs = ob.obs(T, 4, 5, 100, 100)
            for key in OBS_KEYS:
                x = obs[key]
                assert np.array_equal(round_to(x, torch.float16), x.astype(np.float16).view(np.uint16)), key
                u = x.view(np.uint32).astype(np.uint64)
                rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)   # finite values: no NaN here
                assert np.array_equal(round_to(x, torch.bfloat16), rne), key
                seen_inexact |= bool((x.astype(np.float16).astype(np.float32) != x).any())
    assert seen_inexact   # the rollout's quotients do round (the comparison above is not of exact values only)


def _edge_vectors(t, obsT):
    """The oracle's actor vector of agent 0 and critic vector of a reset state, its clock read as t."""
    g = grid("map1.txt")
    H, W = g.shape
    ob = O.OracleBatch(1, g, 3, 5, 2100, seed_base=7, clear_on_reset=False)
    ob.step(np.full((1, 3), 3, np.uint8), auto_reset=False, consts=O.MAPPO_CONSTS)   # stay: the tracker's first update
    oe, ot = ob.env(0), ob.tracker(0)
    rb1, rows = oe.robots1(), ot.rows()
    av = O.generate_vector_features(H, W, t, rb1, rows, 0, obsT, 2, 5)
    _, gv = O.convert_global_state(g, t, rb1, rows, obsT, 100, 100)
    return av, gv


def test_rounding_edge_inputs_are_edges():
    """t / obs_max_time_steps of the edge cases: 257/4096 is a bf16 tie (rounds to even, 0.0625),
    2049/4096 an fp16 tie (rounds to 0.5), 1/50000 an inexact fp16 subnormal (2.0027e-05, not 0)."""
    for vec in _edge_vectors(257, 4096):
        assert vec[-1] == np.float32(257 / 4096) and has_tie(vec, torch.bfloat16)
        assert round_to(vec[-1:], torch.bfloat16)[0] == round_to(np.float32([0.0625]), torch.bfloat16)[0]
    for vec in _edge_vectors(2049, 4096):
        assert vec[-1] == np.float32(2049 / 4096) and has_tie(vec, torch.float16)
        assert round_to(vec[-1:], torch.float16)[0] == np.float16(0.5).view(np.uint16)
    for vec in _edge_vectors(1, 50000):
        assert vec[-1] == np.float32(1) / np.float32(50000) and has_fp16_subnormal(vec)
        h = round_to(vec[-1:], torch.float16).view(np.float16)[0]
        assert h != 0 and abs(float(h) - 2.0027e-05) < 1e-9
    # the predicates do not fire on plain values
    plain = np.float32([0.0, 1.0, -1.0, 0.5, 0.3, 3 / 10, 7 / 19])
    assert not has_tie(plain, torch.bfloat16) and not has_tie(plain, torch.float16)
    assert not has_fp16_subnormal(plain)
    assert not has_fp16_subnormal(np.float32([2.0 ** -15]))   # exact subnormal: a flush is the only way to lose it
    assert not has_tie(np.float32([2.0 ** -20 * (1 + 2.0 ** -11)]), torch.float16)   # below fp16's normal range


@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_half_builders_exist_without_scratch_and_no_other_kernel_is_new(tmp_path):
    """k_obs_small_h<STALE, RL, BF> (8) and k_obs_h<STALE, BF> (4) are in the gfx950 code objects, with
    no private segment and no SGPR spill.  The kernels named k_step* and those of the six launch-matrix
    names are exactly the symbols of tests/step_matrix.py (+ the launch floor) and tests/launch_matrix.py:
    half observations add no step kernel."""
    import launch_matrix
    import step_matrix
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    small = sorted(n for n in res if re.match(r"^_ZN3mdl13k_obs_small_hILb[01]ELb[01]ELb[01]EEE", n))
    gen = sorted(n for n in res if re.match(r"^_ZN3mdl7k_obs_hILb[01]ELb[01]EEE", n))
    assert len(small) == 8 and len(gen) == 4, (small, gen)
    for n in small + gen:
        assert res[n]["private_segment_fixed_size"] == 0, (n, res[n])
        assert res[n].get("sgpr_spill_count", 0) == 0, (n, res[n])
    # the float32 builders keep their symbols
    assert len([n for n in res if re.match(r"^_ZN3mdl11k_obs_smallILb[01]ELb[01]EEE", n)]) == 4
    assert len([n for n in res if re.match(r"^_ZN3mdl5k_obsILb[01]EEE", n)]) == 2
    # each built symbol is one matrix entry's mangled name + template arguments, and there are as many
    step = sorted(n for n in res if "k_step" in n and "k_step_floor" not in n)
    pre = {_mangled_prefix(s) for s in step_matrix.SYMBOLS}
    assert len(step) == len(pre) == len(step_matrix.SYMBOLS) == 96
    assert all(any(n.startswith(p) for p in pre) for n in step), [n for n in step if not any(n.startswith(p) for p in pre)]
    pat = re.compile(r"^_ZN3mdl\d+(?:%s)[IE]" % "|".join(LAUNCH_KERNELS))
    launch = sorted(n for n in res if pat.match(n))
    pre = {_launch_mangled_prefix(s) for s in launch_matrix.SYMBOLS}
    assert len(launch) == len(pre) == len(launch_matrix.SYMBOLS) == 21
    assert all(any(n.startswith(p) for p in pre) for n in launch), launch


def _header_args(name):
    txt = open(HEADER).read()
    m = re.search(rf"^int\s+{name}\((.*?)\);", txt, re.M | re.S)
    assert m, f"{name} not declared in mdl_engine.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append("ptr" if "*" in a else {"int32_t": C.c_int32, "int64_t": C.c_int64}[a.rsplit(" ", 1)[0]])
    return out


@pytest.mark.parametrize("name", NEW)
def test_new_entry_points_header_ctypes_and_exports_agree(name):
    from marl_gpu import _lib
    want = _header_args(name)
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
    # the _as form is the plain entry plus one int32 dtype in front of the observation pointers
    plain = _header_args(name[:-3])
    k = len(want) - 6   # dtype, then the four tensors and the stream
    assert want[:k] + want[k + 1:] == plain and want[k] is C.c_int32


def test_dtype_constants_and_python_defaults():
    from marl_gpu import _lib
    from marl_gpu.engine import OBS_DTYPES, BatchedEnv
    from marl_gpu.rollout import MappoRollout
    txt = open(HEADER).read()
    for nm, v in (("MDL_OBS_F32", 0), ("MDL_OBS_F16", 1), ("MDL_OBS_BF16", 2)):
        assert re.search(rf"^#define {nm} {v}\s*$", txt, re.M), nm
        assert getattr(_lib, nm) == v
    assert OBS_DTYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
    assert set(HALF_DTYPES) | {torch.float32} == set(OBS_DTYPES)
    for fn, par in ((BatchedEnv.obs_buffers, "dtype"), (BatchedEnv.build_obs, "dtype"),
                    (BatchedEnv.step_obs, "obs_dtype"), (MappoRollout.__init__, "obs_dtype")):
        assert inspect.signature(fn).parameters[par].default is torch.float32, fn
    assert "dtype" not in inspect.signature(BatchedEnv.step_episode).parameters   # out of scope: float32 only
