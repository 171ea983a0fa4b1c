"""The map-QMIX cycle collection without a GPU: ``JointReplay.sample`` (the qmix/ trainer's joint
ring, qmix/networks.py:155-239) on CPU tensors filled by hand; the C ABI of the new entry points
(header, ctypes signatures and the built library's exports agree); the CPU-oracle restatement of
the cycle that tests/test_gpu_qmix_cycle.py compares the device against, with the counts that keep
it from being a quiet run; and the new kernels' register budget from the code objects' metadata."""
import ctypes as C
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

from qmix_cycle_ref import CASES, DELIVERING, counts, oracle_cycle  # noqa: E402
from test_host_cpu import LLVM_BIN, _kernel_resources  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdl_engine.h")
NEW = ("mdl_cycle_begin", "mdl_replay_append_joint", "mdl_select_actions_eps_mark", "mdl_select_actions_eps_mark_dev")
OBS, STATE, A = (6, 3, 4), (7, 3, 4), 3


def filled_replay(capacity, n):
    """A ring whose first n rows name their slot: row i holds i everywhere."""
    from marl_gpu.qmix_cycle import JointReplay
    R = JointReplay(capacity, A, OBS, STATE, device="cpu")
    i = torch.arange(n, dtype=torch.float32)
    R.states[:n] = i.reshape(n, 1, 1, 1)
    R.next_states[:n] = i.reshape(n, 1, 1, 1) + 0.25
    R.observations[:n] = i.reshape(n, 1, 1, 1, 1)
    R.next_observations[:n] = i.reshape(n, 1, 1, 1, 1) + 0.5
    R.actions[:n] = (torch.arange(n).reshape(n, 1) + torch.arange(A)) % 15
    R.total_reward[:n, 0] = i * 0.25
    R.dones[:n, 0] = (torch.arange(n) % 3 == 0).to(torch.uint8)
    R.cursor[0] = n % capacity
    R.cursor[1] = n
    return R


def test_ring_tensors_are_the_reference_arrays():
    R = filled_replay(8, 0)
    assert R.states.shape == R.next_states.shape == (8,) + STATE
    assert R.observations.shape == R.next_observations.shape == (8, A) + OBS
    assert R.actions.shape == (8, A) and R.actions.dtype == torch.int64
    assert R.total_reward.shape == (8, 1) and R.total_reward.dtype == torch.float32
    assert R.dones.shape == (8, 1) and R.dones.dtype == torch.uint8
    assert R.cursor.shape == (2,) and R.cursor.dtype == torch.int64
    assert R.state_floats == 7 * 12 and R.obs_floats == 6 * 12


def test_empty_ring():
    R = filled_replay(8, 0)
    assert len(R) == 0 and R.position() == (0, 0) and not R.can_sample(1)
    st, nst, obs, nobs, act, rew, done = R.sample(4)
    assert st.shape == nst.shape == (0,) + STATE and obs.shape == nobs.shape == (0, A) + OBS
    assert act.shape == (0, A) and act.dtype == torch.int64
    assert rew.shape == done.shape == (0, 1) and done.dtype == torch.float32


def test_sample_tuple_order_shapes_dtypes_and_rows():
    R = filled_replay(32, 20)
    assert len(R) == 20 and R.can_sample(20) and not R.can_sample(21)
    st, nst, obs, nobs, act, rew, done = R.sample(8, generator=torch.Generator().manual_seed(3))
    assert st.shape == nst.shape == (8,) + STATE and obs.shape == nobs.shape == (8, A) + OBS
    assert act.shape == (8, A) and rew.shape == done.shape == (8, 1)
    assert all(x.dtype == torch.float32 for x in (st, nst, obs, nobs, rew, done)) and act.dtype == torch.int64
    idx = st[:, 0, 0, 0].long()
    assert len(set(idx.tolist())) == 8 and int(idx.max()) < 20          # distinct stored rows only
    f = idx.float()
    assert torch.equal(st, f.reshape(8, 1, 1, 1).expand(8, *STATE)) and torch.equal(nst, st + 0.25)
    assert torch.equal(obs, f.reshape(8, 1, 1, 1, 1).expand(8, A, *OBS)) and torch.equal(nobs, obs + 0.5)
    assert torch.equal(act, (idx.reshape(8, 1) + torch.arange(A)) % 15)
    assert torch.equal(rew[:, 0], f * 0.25) and torch.equal(done[:, 0], (idx % 3 == 0).float())
    again = R.sample(8, generator=torch.Generator().manual_seed(3))
    assert torch.equal(again[0], st)                                     # the generator decides the draw
    assert sorted(R.sample(20)[0][:, 0, 0, 0].tolist()) == list(range(20))


def test_fewer_rows_than_batch_returns_all_in_order():
    R = filled_replay(32, 5)
    st, nst, obs, nobs, act, rew, done = R.sample(16)
    assert st.shape == (5,) + STATE and st[:, 0, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert act[:, 0].tolist() == [0, 1, 2, 3, 4] and done[:, 0].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0]


def test_full_ring_samples_every_slot_and_bad_sizes():
    from marl_gpu.qmix_cycle import JointReplay
    R = filled_replay(12, 12)
    assert R.position() == (0, 12)
    assert sorted(R.sample(12)[5][:, 0].tolist()) == [i * 0.25 for i in range(12)]
    with pytest.raises(ValueError):
        JointReplay(0, A, OBS, STATE, device="cpu")
    with pytest.raises(ValueError):
        JointReplay(4, 0, OBS, STATE, device="cpu")


# ---- C ABI of the new entry points: header == ctypes signatures == exported symbols
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def header_args(name):
    txt = open(HEADER).read()
    m = re.search(rf"^int\s+{name}\(([^;]*?)\);", txt, re.M | re.S)
    assert m, f"{name} is not declared in include/mdl_engine.h"
    args = []
    for a in m.group(1).split(","):
        a = re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip()
        if "*" in a:
            args.append("ptr")
        else:
            args.append(CTYPE[a.replace("const ", "").split()[0]])
    return args


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


# ---- the oracle side of the cycle test: not a quiet run
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_cycle_counts(name):
    case = CASES[name]
    E = case["cfg"][4]
    recs = list(oracle_cycle(case))
    assert len(recs) == case["steps"]
    got = counts(recs, E)
    assert got == case["counts"], f"{name}: (mixed, none, at T, deliveries, pick-ups) = {got}"
    assert got[0] >= 1 and got[1] >= 1 and got[2] >= 1 and got[4] >= 1
    assert got[3] >= 1 or name not in DELIVERING      # see qmix_cycle_ref.CASES on the specified runs' deliveries
    for k, envs in case["marks"].items():                 # a forced mark cuts an episode before its time limit
        assert all(recs[k]["marked"][e] and recs[k]["completed_steps"][e] < case["cfg"][3] for e in envs)
    assert any(r["completed_return"].any() for r in recs)


# ---- register budget of the new kernels
@pytest.mark.skipif(not os.path.exists(f"{LLVM_BIN}/llvm-readelf"), reason="ROCm LLVM tools absent")
def test_new_kernels_use_no_scratch_and_spill_no_sgpr(tmp_path):
    from marl_gpu import _lib
    res = _kernel_resources(_lib.LIB_PATH, tmp_path)
    begin = {k: v for k, v in res.items() if "k_cycle_begin" in k}
    copy = {k: v for k, v in res.items() if "k_replay_copy_joint" in k}
    assert len(begin) == 10, sorted(begin)      # <STALE> x <NCH = 1, 2, 4, 8, 16>
    assert len(copy) == 2, sorted(copy)         # vector and scalar rows
    for k, v in {**begin, **copy}.items():
        assert v["private_segment_fixed_size"] == 0, f"{k} uses scratch: {v}"
        assert v.get("sgpr_spill_count", 0) == 0, f"{k} spills SGPRs: {v}"
    assert not any("k_step" in k for k in list(begin) + list(copy))
