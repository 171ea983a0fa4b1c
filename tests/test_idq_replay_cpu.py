"""``TransitionReplay`` (IDQ's per-transition ring, IDQ/networks.py:46-104) on CPU tensors filled
by hand: the sample tuple's shapes and dtypes, sampling without replacement, the
fewer-than-batch rule; and the C ABI of the IDQ collection entry points: header, ctypes
signatures and the built library's exports agree.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mdl_engine.h")
NEW = ("mdl_alt_pre_bytes", "mdl_alt_transition", "mdl_replay_append")


def filled_replay(capacity, n, obs_shape=(6, 3, 4)):
    """A ring whose first n rows name their slot: row i holds i everywhere."""
    from marl_gpu.idq_rollout import TransitionReplay
    R = TransitionReplay(capacity, obs_shape, device="cpu")
    i = torch.arange(n, dtype=torch.float32)
    R.observations[:n] = i.reshape(n, 1, 1, 1)
    R.next_observations[:n] = i.reshape(n, 1, 1, 1) + 0.5
    R.actions[:n] = torch.arange(n) % 15
    R.rewards[:n] = i * 0.25
    R.dones[:n] = (torch.arange(n) % 3 == 0).to(torch.uint8)
    R.cursor[0] = n % capacity
    R.cursor[1] = n
    return R


def test_empty_ring():
    R = filled_replay(8, 0)
    assert len(R) == 0 and R.position() == (0, 0) and not R.can_sample(1)
    obs, act, rew, nxt, done = R.sample(4)
    assert obs.shape == (0, 6, 3, 4) and act.shape == (0,) and act.dtype == torch.int64 and done.dtype == torch.float32


def test_sample_shapes_dtypes_and_rows():
    R = filled_replay(32, 20)
    assert len(R) == 20 and R.can_sample(20) and not R.can_sample(21)
    g = torch.Generator().manual_seed(3)
    obs, act, rew, nxt, done = R.sample(8, generator=g)
    assert obs.shape == nxt.shape == (8, 6, 3, 4) and obs.dtype == nxt.dtype == torch.float32
    assert act.shape == rew.shape == done.shape == (8,)
    assert act.dtype == torch.int64 and rew.dtype == torch.float32 and done.dtype == torch.float32
    idx = obs[:, 0, 0, 0].long()
    assert len(set(idx.tolist())) == 8 and int(idx.max()) < 20          # distinct stored rows only
    assert torch.equal(obs, idx.float().reshape(8, 1, 1, 1).expand(8, 6, 3, 4))
    assert torch.equal(nxt, obs + 0.5) and torch.equal(act, idx % 15) and torch.equal(rew, idx.float() * 0.25)
    assert torch.equal(done, (idx % 3 == 0).float())
    again = R.sample(8, generator=torch.Generator().manual_seed(3))
    assert torch.equal(again[0], obs)                                    # the generator decides the draw
    assert sorted(R.sample(20)[0][:, 0, 0, 0].tolist()) == list(range(20))


def test_fewer_rows_than_batch_returns_all_in_order():
    R = filled_replay(32, 5)
    obs, act, rew, nxt, done = R.sample(16)
    assert obs.shape == (5, 6, 3, 4) and obs[:, 0, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert act.tolist() == [0, 1, 2, 3, 4] and done.tolist() == [1.0, 0.0, 0.0, 1.0, 0.0]


def test_full_ring_samples_every_slot():
    R = filled_replay(12, 12)
    assert R.position() == (0, 12)
    assert sorted(R.sample(12)[2].tolist()) == [i * 0.25 for i in range(12)]


def test_int_obs_shape_and_bad_capacity():
    from marl_gpu.idq_rollout import TransitionReplay
    R = TransitionReplay(4, 7, device="cpu")
    assert R.observations.shape == (4, 7) and R.row_floats == 7
    with pytest.raises(ValueError):
        TransitionReplay(0, 7, device="cpu")


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


def test_replay_bound_matches_header():
    from marl_gpu import _lib
    m = re.search(r"^#define\s+MDL_REPLAY_MAX_ENVS\s+(\d+)", open(HEADER).read(), re.M)
    assert m and int(m.group(1)) == _lib.MDL_REPLAY_MAX_ENVS
