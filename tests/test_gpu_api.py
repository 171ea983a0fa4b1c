"""Argument checking at the tensor API and the dict API:
env-id subsets, caller-owned output buffers, observation ranges over mixed map
shapes, and the reference's list semantics for repeated / negative indices in
``VectorizedEnv`` (QMIX/env_vectorized.py:13-37)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from golden_io import grid  # noqa: E402


def _mg():
    import marl_gpu
    return marl_gpu


def snap(env):
    s = env.read_state()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in s.items()}


def test_host_env_ids_checked_like_list_indexing():
    mg = _mg()
    E, A = 8, 5
    env = mg.BatchedEnv(grid("map1.txt"), E, A, 20, 50, seed=3)
    env.reset()
    acts = torch.randint(0, 15, (2, A), dtype=torch.uint8, device="cuda")
    with pytest.raises(IndexError):
        env.step(acts, env_ids=[0, 8])
    with pytest.raises(IndexError):
        env.step(acts, env_ids=[-9, 1])
    with pytest.raises(ValueError, match="duplicate"):
        env.step(acts, env_ids=[3, 3])
    with pytest.raises(IndexError):
        env.reset([E])
    with pytest.raises(TypeError):
        env.reset([0.5])
    # negative ids count from the end: [-1, 2] == [7, 2]
    twin = mg.BatchedEnv(grid("map1.txt"), E, A, 20, 50, seed=3)
    twin.reset()
    r1, _, _ = env.step(acts, env_ids=[-1, 2])
    r1 = r1.clone()
    r2, _, _ = twin.step(acts, env_ids=np.array([7, 2]))
    assert torch.equal(r1, r2)
    s1, s2 = snap(env), snap(twin)
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    # an empty subset is a no-op (an empty id tensor must not read as "all envs")
    before = snap(env)
    r, sh, d = env.step(torch.empty((0, A), dtype=torch.uint8, device="cuda"), env_ids=[])
    assert r.numel() == 0
    env.reset([])
    after = snap(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_device_env_ids_out_of_range_are_skipped():
    """Device-side ids are not read back on the host; an id outside [0, E) is skipped by
    the kernels instead of writing another env's (or another allocation's) memory."""
    mg = _mg()
    E, A = 8, 5
    env = mg.BatchedEnv(grid("map1.txt"), E, A, 20, 50, seed=5)
    env.reset()
    before = snap(env)
    ids = torch.tensor([E, 1 << 20, -3], dtype=torch.int32, device="cuda")
    env.step(torch.randint(0, 15, (3, A), dtype=torch.uint8, device="cuda"), env_ids=ids)
    env.reset(ids)
    env.clear_tracker(ids)
    after = snap(env)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_out_buffers_checked():
    mg = _mg()
    E, A = 16, 5
    env = mg.BatchedEnv(grid("map1.txt"), E, A, 20, 50, seed=1)
    env.reset()
    acts = torch.randint(0, 15, (E, A), dtype=torch.uint8, device="cuda")
    f64 = torch.zeros(E, dtype=torch.float64, device="cuda")
    f32 = torch.zeros(E, dtype=torch.float32, device="cuda")
    u8 = torch.zeros(E, dtype=torch.uint8, device="cuda")
    env.step(acts, out=(f64, f32, u8))
    with pytest.raises(TypeError):
        env.step(acts, out=(f32, f32, u8))
    with pytest.raises(ValueError, match="needs 16"):
        env.step(acts, out=(f64[:8], f32, u8))
    with pytest.raises(ValueError):
        env.step(acts, out=(f64.cpu(), f32, u8))
    with pytest.raises(ValueError):
        env.step(acts[:3])
    with pytest.raises(ValueError):
        env.step_fused(acts.view(1, E, A), out=(f64, f32, u8[:4]))


def test_obs_range_must_not_mix_map_shapes():
    mg = _mg()
    maps = [grid("map1.txt"), grid("map2.txt"), grid("map3.txt")]
    env_map = [0] * 4 + [1] * 3 + [2] * 3       # 10x10, then 20x20 (map2, map3 share a shape)
    env = mg.BatchedEnv(maps, 10, 5, 20, 50, seed=1, env_map=env_map)
    env.reset()
    with pytest.raises(ValueError, match="mix map shapes"):
        env.build_obs()                           # whole batch: 10x10 and 20x20
    with pytest.raises(ValueError, match="mix map shapes"):
        env.build_obs(2, 4)
    with pytest.raises(ValueError, match="mix map shapes"):
        env.build_obs_alt()
    a = env.build_obs(0, 4)
    assert a["actor_map"].shape == (4, 5, 6, 10, 10)
    b = env.build_obs(4, 6)                       # map2 + map3: one 20x20 run
    assert b["critic_map"].shape == (6, 4, 20, 20)
    with pytest.raises(ValueError, match="needs"):
        env.build_obs(4, 6, out=a)                # 10x10 buffers for 20x20 envs
    with pytest.raises(IndexError):
        env.build_obs(8, 5)
    # the C ABI refuses a mixed range on its own (not only the Python layer)
    lib = mg.lib()
    import ctypes as C
    rc = lib.mdl_build_obs(env._h, 0, 10, None, None, None, None, C.c_void_p(0))
    assert rc != 0 and b"mix map shapes" in lib.mdl_last_error()


def test_vectorized_env_repeated_and_negative_indices():
    """The reference steps ``self.envs[i]`` in list order: an env listed twice steps
    twice (the second result sees the first), a negative index counts from the end."""
    from marl_gpu.compat import VectorizedEnv
    kw = dict(map_file="map1.txt", n_robots=3, n_packages=10, max_time_steps=30, seed=11)
    v1 = VectorizedEnv(None, 4, **kw)
    v2 = VectorizedEnv(None, 4, **kw)
    v1.reset()
    v2.reset()
    rs = np.random.RandomState(0)
    moves, ops = ["S", "L", "R", "U", "D"], ["0", "1", "2"]
    for _ in range(10):
        acts = [[(moves[rs.randint(5)], ops[rs.randint(3)]) for _ in range(3)] for _ in range(3)]
        s1, r1, d1, i1 = v1.step(acts, indices=[2, -2, 2])
        # the same as three single-env calls in order
        want = [v2.step([acts[0]], indices=[2]), v2.step([acts[1]], indices=[2]), v2.step([acts[2]], indices=[2])]
        for k in range(3):
            assert s1[k] == want[k][0][0]
            assert r1[k] == want[k][1][0]
            assert d1[k] == want[k][2][0]
            assert i1[k] == want[k][3][0]
    with pytest.raises(IndexError):
        v1.step([[("S", "0")] * 3], indices=[4])
    # zip semantics: more indices than actions steps only as many envs as there are actions
    s, r, d, i = v1.step([[("S", "0")] * 3], indices=[0, 1])
    assert len(s) == 1
    # ... and an index past the end of the action list is never looked up (zip), even out of range
    s, r, d, i = v1.step([[("S", "0")] * 3], indices=[0, 99])
    assert len(s) == 1
    st = v1.reset(indices=[1, 1])
    assert len(st) == 2


# (map, A, P, tracker, layout, with_obs, symbol): the step dispatch written out by hand -- STALE from
# the tracker, NCH = chunks of 64 packages rounded up to 1, 2, 4, 8, 16, then AU = A for A = 5 / 16
# up to two chunks, else 8 for A <= 8, else 0; rows: AU 5 or 8, NFULL 3 from P = 48; halves: NFULL 3
# from P = 96; the fused step + observation kernel: AU 5 or 8
KERNEL_NAMES = [
    ("map1.txt", 5, 50, "mappo", "wave", False, "mdl::k_step<true, 1, false, 5>"),
    ("map2.txt", 16, 100, "mappo", "wave", False, "mdl::k_step<true, 2, false, 16>"),
    ("map1.txt", 3, 10, "fresh", "wave", False, "mdl::k_step<false, 1, false, 8>"),
    ("map2.txt", 5, 200, "mappo", "wave", False, "mdl::k_step<true, 4, false, 8>"),
    ("map2.txt", 20, 300, "fresh", "wave", False, "mdl::k_step<false, 8, false, 0>"),
    ("map1.txt", 9, 600, "mappo", "wave", False, "mdl::k_step<true, 16, false, 0>"),
    ("map1.txt", 8, 128, "fresh", "wave", False, "mdl::k_step<false, 2, false, 8>"),
    ("map2.txt", 16, 129, "mappo", "wave", False, "mdl::k_step<true, 4, false, 0>"),
    ("map2.txt", 8, 40, "fresh", "rows", False, "mdl::k_step_rows<false, 8, 4, 0>"),
    ("map1.txt", 5, 48, "mappo", "rows", False, "mdl::k_step_rows<true, 5, 4, 3>"),
    ("map1.txt", 5, 47, "mappo", "rows", False, "mdl::k_step_rows<true, 5, 4, 0>"),
    ("map2.txt", 16, 95, "fresh", "halves", False, "mdl::k_step_halves<false, 0>"),
    ("map2.txt", 16, 96, "mappo", "halves", False, "mdl::k_step_halves<true, 3>"),
    ("map1.txt", 4, 20, "fresh", "wave", True, "mdl::k_step_obs<false, 8>"),
    ("map1.txt", 5, 64, "mappo", "wave", True, "mdl::k_step_obs<true, 5>"),
]


@pytest.mark.parametrize("mapname,A,P,tracker,layout,with_obs,want", KERNEL_NAMES,
                         ids=[f"A{c[1]}-P{c[2]}-{c[3]}-{'obs' if c[5] else c[4]}" for c in KERNEL_NAMES])
def test_step_kernel_name_table(mapname, A, P, tracker, layout, with_obs, want):
    """The symbol the engine reports for a step launch (what bench.py labels its roofline record
    with) against the dispatch rule written out as literals; no stepping."""
    env = _mg().BatchedEnv(grid(mapname), 8, A, P, 20, seed=1, tracker=tracker, max_packages_obs=5)
    assert env.step_kernel_name(layout, with_obs=with_obs) == want
    env.close()


# What the parent of the shared buffer check raised, by the way a caller's buffer is wrong: a wrong
# dtype, a non-contiguous view, one entry too few, a CPU tensor.  Read off each call site as it stood
# before the checks were unified (every one of them is refused in Python, before any launch).
_T, _V = TypeError, ValueError
MASK_ERRS = dict(dtype=_T, noncontig=_V, short=_V, cpu=_V)      # uint8 [E] masks; episode_results' outputs
OBS_ERRS = dict(dtype=_T, noncontig=_T, short=_V, cpu=_T)       # observation outputs; alt_transition's pre
ALL_TYPE = dict(dtype=_T, noncontig=_T, short=_T, cpu=_T)       # r_out, completed_return, completed_steps
ALL_VALUE = dict(dtype=_V, noncontig=_V, short=_V, cpu=_V)      # greedy_actions*' and avail_actions' out


def _bad_buffers(good):
    """The four wrong forms of a valid caller buffer."""
    return dict(dtype=good.to(torch.int16), noncontig=torch.stack([good, good], dim=-1)[..., 0],
                short=good.reshape(-1)[:-1], cpu=good.cpu())


def test_caller_buffers_refused_as_before():
    """Every public BatchedEnv method that takes a caller buffer, offered each buffer in the four
    wrong forms: refused with the exception type its call site has always raised."""
    E, A, P = 3, 2, 3
    env = _mg().BatchedEnv(grid("map1.txt"), E, A, P, 20, seed=1)
    H, W = env.single_map_shape("test")
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device="cuda")   # noqa: E731
    acts = z(E, A)
    obs = env.obs_buffers()
    alt = dict(idq_obs=z(E, A, 6, H, W, dt=torch.float32), qmix_state=z(E, 7, H, W, dt=torch.float32))
    res = (z(E, dt=torch.float64), z(E, dt=torch.int32), z(E, dt=torch.int32))
    pre, done = env.alt_pre_buffer(), z(E)

    def with_res(i, t):
        return tuple(t if k == i else r for k, r in enumerate(res))

    # (what is offered, the valid buffer, the call with a replacement for it, the parent's exceptions)
    table = []
    for k in obs:
        table += [(f"step_obs obs_out[{k}]", obs[k], lambda t, k=k: env.step_obs(acts, obs_out={**obs, k: t}), OBS_ERRS),
                  (f"step_episode obs_out[{k}]", obs[k],
                   lambda t, k=k: env.step_episode(acts, z(E), obs_out={**obs, k: t}), OBS_ERRS),
                  (f"build_obs out[{k}]", obs[k], lambda t, k=k: env.build_obs(out={**obs, k: t}), OBS_ERRS)]
    for k in alt:
        table += [(f"build_obs_alt out[{k}]", alt[k], lambda t, k=k: env.build_obs_alt(out={**alt, k: t}), OBS_ERRS)]
    table += [
        ("step_episode active", z(E), lambda t: env.step_episode(acts, t), MASK_ERRS),
        ("step_episode filled", z(E), lambda t: env.step_episode(acts, z(E), filled=t), MASK_ERRS),
        ("alt_transition pre", pre, lambda t: env.alt_transition(acts, t), OBS_ERRS),
        ("alt_transition row_mask", z(E), lambda t: env.alt_transition(acts, pre, row_mask=t), MASK_ERRS),
        ("alt_transition r_out", z(E, A, dt=torch.float64), lambda t: env.alt_transition(acts, pre, r_out=t), ALL_TYPE),
        ("cycle_begin done", done, lambda t: env.cycle_begin(t), MASK_ERRS),
        ("cycle_begin completed", z(E), lambda t: env.cycle_begin(done, completed=t), MASK_ERRS),
        ("cycle_begin completed_return", res[0], lambda t: env.cycle_begin(done, completed_return=t), ALL_TYPE),
        ("cycle_begin completed_steps", res[1], lambda t: env.cycle_begin(done, completed_steps=t), ALL_TYPE),
        ("greedy_actions out", z(E, A), lambda t: env.greedy_actions(out=t), ALL_VALUE),
        ("greedy_actions_masked active", z(E), lambda t: env.greedy_actions_masked(t), MASK_ERRS),
        ("greedy_actions_masked out", z(E, A), lambda t: env.greedy_actions_masked(z(E), out=t), ALL_VALUE),
        ("avail_actions active", z(E), lambda t: env.avail_actions(t), MASK_ERRS),
        ("avail_actions out", z(E, A, 15), lambda t: env.avail_actions(out=t), ALL_VALUE),
    ]
    for i, name in enumerate(("total_reward", "delivered", "steps")):
        table += [(f"episode_results out {name}", res[i], lambda t, i=i: env.episode_results(with_res(i, t)), MASK_ERRS)]
    wrong = []
    for what, good, call, errs in table:
        for case, t in _bad_buffers(good).items():
            try:
                call(t)
                got = None
            except Exception as e:   # noqa: BLE001 -- the type is what is under test
                got = type(e)
            if got is not errs[case]:
                wrong.append(f"{what}, {case}: {getattr(got, '__name__', got)}, not {errs[case].__name__}")
    assert not wrong, "\n".join(wrong)
    env.close()
