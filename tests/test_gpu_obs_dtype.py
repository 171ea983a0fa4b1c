"""Half-precision observations on the device: BatchedEnv.build_obs(dtype=), step_obs(obs_dtype=) and
MappoRollout(obs_dtype=) for torch.float16 and torch.bfloat16.  The contract: every element is the
float32 value the engine writes, rounded once to nearest-even -- compared as bit patterns with torch's
CPU conversion of the float32 build (obs_dtype_ref.round_to), ties, zero signs and fp16 subnormals
included -- from both builders, at any 2-byte alignment, for env sub-ranges, and pinned to the oracle."""
import numpy as np
import pytest
import torch

import oracle as O
from golden_io import grid
from obs_dtype_ref import HALF_DTYPES, OBS_KEYS, bits16, has_fp16_subnormal, has_tie, round_to
from test_gpu_obs_small import CASES

pytestmark = pytest.mark.gpu

DT_IDS = ["fp16", "bf16"]
STAY = 3   # trainer int: move S, no package op


def _mg():
    import marl_gpu
    return marl_gpu


def _acts(gen, E, A):
    return torch.from_numpy(gen.randint(0, 15, size=(E, A)).astype(np.uint8)).cuda()


def _assert_rounded(half, f32, dtype, what):
    """Every tensor of the half dict is bit for bit the float32 one converted on the CPU."""
    for key in OBS_KEYS:
        h, x = half[key], f32[key]
        assert h.dtype == dtype and tuple(h.shape) == tuple(x.shape), (key, what)
        got, want = bits16(h), round_to(x.cpu().numpy(), dtype)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            i = tuple(bad[0])
            raise AssertionError(f"{key} {what}: {len(bad)} elements differ, first at {i}: got 0x{got[i]:04x}, "
                                 f"want 0x{want[i]:04x} (float32 {x.cpu().numpy()[i]!r})")


# ---- 1. half builds against the float32 build: both builders, the shapes of test_gpu_obs_small ----
@pytest.mark.parametrize("builder", ["auto", "generic"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-A{c[1]}-P{c[2]}-{c[4]}" for c in CASES])
def test_half_build_is_the_rounded_float32_build(case, builder):
    mg = _mg()
    m, A, P, T, tracker, MO, MP, MR, MPs, obsT = case
    g = grid(m)
    E = 37   # a last partial workgroup
    env = mg.BatchedEnv(g, E, A, P, T, seed=11, tracker=tracker, max_other_robots=MO, max_packages_obs=MP,
                        max_robots_state=MR, max_packages_state=MPs, obs_max_time_steps=obsT, obs_builder=builder)
    env.reset()
    gen = np.random.RandomState(5)
    inexact = False
    for k in range(T + 9):   # across the auto-resets at t = T
        env.step(_acts(gen, E, A))
        if k % 13 == 4 or k == T + 8:
            ref = env.build_obs()
            for dt in HALF_DTYPES:
                _assert_rounded(env.build_obs(dtype=dt), ref, dt, f"step {k} {builder}")
            v = ref["actor_vec"].cpu().numpy()
            inexact |= bool((v.astype(np.float16).astype(np.float32) != v).any())
    assert inexact   # the builds held values that do round
    env.close()


# ---- 2. against the oracle directly, config 3 sizes ----
@pytest.mark.parametrize("dtype", HALF_DTYPES, ids=DT_IDS)
def test_half_build_config3_vs_oracle(dtype):
    mg = _mg()
    g = grid("map1.txt")
    E, A, P, T = 16, 5, 50, 40
    env = mg.BatchedEnv(g, E, A, P, T, seed=42, tracker="mappo", max_other_robots=4, max_packages_obs=5)
    env.reset()
    ob = O.OracleBatch(E, g, A, P, T, seed_base=42, clear_on_reset=False)
    gen = np.random.RandomState(3)
    for k in range(90):
        ints = gen.randint(0, 15, size=(E, A)).astype(np.uint8)
        env.step(torch.from_numpy(ints).cuda())
        ob.step(ints, auto_reset=True, consts=O.MAPPO_CONSTS)
        if k % 15 == 7:
            o = env.build_obs(dtype=dtype)
            want = ob.obs(T, 4, 5, 100, 100)
            for key in OBS_KEYS:
                assert np.array_equal(bits16(o[key]), round_to(want[key], dtype)), (key, k)
    env.close()


# ---- 3. alignment and range ----
@pytest.mark.parametrize("dtype", HALF_DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [("map.txt", 4, 20, 30, 6, 8, 3, 10), ("map1.txt", 5, 50, 60, 100, 100, 100, 100),
                                  ("map4.txt", 3, 30, 40, 2, 5, 4, 7)],
                         ids=["7x7", "config3b", "19x20"])
@pytest.mark.parametrize("builder", ["auto", "generic"])
def test_half_emission_any_alignment_and_range(case, dtype, builder):
    """Every element of each tensor is written exactly once wherever the tensor starts inside a 16-B
    line (1..7 elements in), for env sub-ranges, with 16-B groups that straddle envs / planes / agents:
    the rounded float32 build, the sentinels around each tensor intact.  Both builders: the general one's
    half emitters (emit_h, the eight-per-lane map forms and their element-wise fallback) take the same
    heads and tails."""
    mg = _mg()
    m, A, P, T, MO, MP, MR, MPs = case
    g = grid(m)
    E = 37
    env = mg.BatchedEnv(g, E, A, P, T, seed=3, tracker="mappo", max_other_robots=MO, max_packages_obs=MP,
                        max_robots_state=MR, max_packages_state=MPs, obs_builder=builder)
    env.reset()
    gen = np.random.RandomState(8)
    for _ in range(T // 2 + 3):
        env.step(_acts(gen, E, A))
    ref = {k: round_to(v.cpu().numpy(), dtype) for k, v in env.build_obs().items()}
    shapes = {k: v.shape for k, v in ref.items()}
    sentinel = torch.tensor(-7.0, dtype=dtype)
    sbits = int(bits16(sentinel.reshape(1))[0])
    for lead in range(1, 8):
        for b, n in ((0, E), (5, 20), (36, 1)):
            out, raw = {}, {}
            for k, shp in shapes.items():
                cnt = int(np.prod((n,) + shp[1:]))
                buf = torch.full((lead + cnt + 9,), -7.0, dtype=dtype, device="cuda")
                assert buf.data_ptr() % 16 == 0
                raw[k] = buf
                out[k] = buf[lead:lead + cnt].view((n,) + shp[1:])
            env.build_obs(env_begin=b, n=n, out=out, dtype=dtype)
            torch.cuda.synchronize()
            for k in shapes:
                got = bits16(out[k])
                assert np.array_equal(got, ref[k][b:b + n]), (k, lead, b, n)
                r = bits16(raw[k])
                assert (r[:lead] == sbits).all() and (r[lead + got.size:] == sbits).all(), (k, lead, b, n)
    # one tensor alone (the others not requested)
    o = env.build_obs(which=("critic_vec",), dtype=dtype)
    assert np.array_equal(bits16(o["critic_vec"]), ref["critic_vec"])
    o = env.build_obs(which=("actor_map",), dtype=dtype)
    assert np.array_equal(bits16(o["actor_map"]), ref["actor_map"])
    env.close()


# ---- 4. rounding edges on the device ----
@pytest.mark.parametrize("builder", ["auto", "generic"])
def test_rounding_edges_on_the_device(builder):
    """t / obs_max_time_steps at a bf16 tie (257/4096), an fp16 tie (2049/4096) and an inexact fp16
    subnormal (1/50000): the float32 build holds the edge, the half builds equal the reference."""
    mg = _mg()
    g = grid("map1.txt")
    E, A, P, T = 4, 3, 5, 2100
    stay = torch.full((E, A), STAY, dtype=torch.uint8, device="cuda")
    env = mg.BatchedEnv(g, E, A, P, T, seed=9, tracker="mappo", max_other_robots=2, max_packages_obs=5,
                        obs_max_time_steps=4096, obs_builder=builder)
    env.reset()
    t = 0
    for stop, dt in ((257, torch.bfloat16), (2049, torch.float16)):
        while t < stop:
            env.step(stay, auto_reset=False)
            t += 1
        assert int(env.read_state()["t"].min()) == int(env.read_state()["t"].max()) == stop
        ref = env.build_obs()
        for key in ("actor_vec", "critic_vec"):
            assert has_tie(ref[key].cpu().numpy(), dt), (key, stop)
        for d in HALF_DTYPES:
            _assert_rounded(env.build_obs(dtype=d), ref, d, f"t={stop}")
    env.close()
    env = mg.BatchedEnv(g, E, A, P, T, seed=9, tracker="mappo", max_other_robots=2, max_packages_obs=5,
                        obs_max_time_steps=50000, obs_builder=builder)
    env.reset()
    env.step(stay, auto_reset=False)
    ref = env.build_obs()
    for key in ("actor_vec", "critic_vec"):
        assert has_fp16_subnormal(ref[key].cpu().numpy()), key
    half = env.build_obs(dtype=torch.float16)
    _assert_rounded(half, ref, torch.float16, "t=1 of 50000")
    assert float(half["critic_vec"][0, -1]) != 0.0   # not flushed
    _assert_rounded(env.build_obs(dtype=torch.bfloat16), ref, torch.bfloat16, "t=1 of 50000")
    env.close()


# ---- 5. step_obs(obs_dtype=) ----
@pytest.mark.parametrize("dtype", HALF_DTYPES, ids=DT_IDS)
def test_step_obs_half_steps_like_float32(dtype):
    mg = _mg()
    g = grid("map1.txt")
    E, A, P, T = 21, 5, 30, 12
    kw = dict(seed=4, tracker="mappo", shaping="mappo", max_other_robots=4, max_packages_obs=5)
    a, b = mg.BatchedEnv(g, E, A, P, T, **kw), mg.BatchedEnv(g, E, A, P, T, **kw)
    a.reset()
    b.reset()
    gen = np.random.RandomState(6)
    for k in range(2 * T):
        acts = _acts(gen, E, A)
        ra, sa, da, oa = a.step_obs(acts)
        rb, sb, db, ob = b.step_obs(acts, obs_dtype=dtype)
        assert torch.equal(ra, rb) and torch.equal(da, db), k
        assert np.array_equal(sa.cpu().numpy().view(np.uint32), sb.cpu().numpy().view(np.uint32)), k
        _assert_rounded(ob, oa, dtype, f"step {k}")
    sa, sb = a.read_state(), b.read_state()
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    # the float32 call on the same engine afterwards still uses its own (float32) cached buffers
    assert b.step_obs(acts)[3]["actor_vec"].dtype == torch.float32
    a.close()
    b.close()


# ---- 6. MappoRollout(obs_dtype=) ----
@pytest.mark.parametrize("dtype", HALF_DTYPES, ids=DT_IDS)
def test_mappo_rollout_half_observations(dtype):
    """The half rollout's networks compute on x.float(); a float32 twin's on x.to(D).float(): the same
    numbers, so actions, log-probs, values' consequences (advantages, returns), rewards and dones match
    bitwise, and the half buffers are the twin's rounded ones.  graph=True replays equal eager calls."""
    mg = _mg()
    from marl_gpu.rollout import MappoRollout
    g = grid("map1.txt")
    E, A, P, T, steps = 8, 5, 30, 6, 10   # T < steps: auto-resets inside the rollout

    def make():
        env = mg.BatchedEnv(g, E, A, P, T, seed=7, tracker="mappo", shaping="mappo", max_other_robots=A - 1,
                            max_packages_obs=5)
        env.reset()
        return env

    gen = torch.Generator(device="cuda").manual_seed(3)
    envs = [make() for _ in range(3)]
    wa = torch.randn(envs[0].actor_vec_dim, 15, device="cuda", generator=gen)
    wc = torch.randn(envs[0].critic_vec_dim, device="cuda", generator=gen) * 0.01

    def actor(obs, vec):    # (float32 inputs: the conversions below are then the identity / the rounding)
        obs, vec = obs.to(dtype).float(), vec.to(dtype).float()
        return vec @ wa * 0.1 + obs.sum(dim=(1, 2, 3)).unsqueeze(1) * 0.01

    def critic(gmap, gvec):
        return gvec.to(dtype).float() @ wc + gmap.to(dtype).float().sum(dim=(1, 2, 3)) * 0.001

    half = MappoRollout(envs[0], steps, seed=5, obs_dtype=dtype)
    twin = MappoRollout(envs[1], steps, seed=5)
    graphed = MappoRollout(envs[2], steps, seed=5, obs_dtype=dtype)
    for k in ("mb_obs", "mb_vector_obs", "mb_global_states", "mb_global_vector"):
        assert getattr(half, k).dtype == dtype and getattr(twin, k).dtype == torch.float32
    assert all(v.dtype == dtype for v in half.next_obs.values())
    for k in ("mb_log_probs", "mb_rewards", "mb_values"):
        assert getattr(half, k).dtype == torch.float32
    for call in range(3):   # call 0 captures; calls 1, 2 replay
        h = [x.clone() for x in half.collect(actor, critic)]
        w = [x.clone() for x in twin.collect(actor, critic)]
        gr = [x.clone() for x in graphed.collect(actor, critic, graph=True)]
        for i in range(4):   # the observation buffers
            assert h[i].dtype == dtype and np.array_equal(bits16(h[i]), round_to(w[i].cpu().numpy(), dtype)), (call, i)
        for i in range(4, 9):   # actions, log-probs, advantages, returns, rewards
            assert h[i].dtype == w[i].dtype and torch.equal(h[i], w[i]), (call, i)
        assert torch.equal(half.mb_dones, twin.mb_dones) and bool(half.mb_dones.any()), call
        assert torch.equal(half.mb_values, twin.mb_values), call
        for key in OBS_KEYS:
            assert np.array_equal(bits16(half.next_obs[key]), round_to(twin.next_obs[key].cpu().numpy(), dtype)), key
        for i, (x, y) in enumerate(zip(h, gr)):
            assert x.dtype == y.dtype and torch.equal(x, y), f"rollout {call}, output {i}: replay != eager"
    assert envs[0].save_state().tobytes() == envs[1].save_state().tobytes() == envs[2].save_state().tobytes()
    for e in envs:
        e.close()


# ---- 7. argument checks ----
def test_dtype_argument_checks():
    mg = _mg()
    from marl_gpu import _lib
    g = grid("map1.txt")
    E, A, P, T = 4, 3, 5, 20
    env = mg.BatchedEnv(g, E, A, P, T, seed=1, tracker="mappo", max_other_robots=2, max_packages_obs=5)
    env.reset()
    f32 = env.obs_buffers()
    bf = env.obs_buffers(dtype=torch.bfloat16)
    assert all(v.dtype == torch.bfloat16 for v in bf.values())
    with pytest.raises(TypeError):
        env.build_obs(out=f32, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        env.build_obs(out=bf, dtype=torch.float32)
    with pytest.raises(TypeError, match="float32"):
        env.build_obs(out=bf)   # no dtype given: the float32 contract, as before
    with pytest.raises(TypeError):
        env.build_obs(out=bf, dtype=torch.float16)
    for bad in (torch.float64, torch.int16, None):
        with pytest.raises(TypeError):
            env.build_obs(dtype=bad)
        with pytest.raises(TypeError):
            env.obs_buffers(dtype=bad)
    acts = torch.full((E, A), STAY, dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        env.step_obs(acts, obs_dtype=torch.float64)
    with pytest.raises(TypeError):
        env.step_obs(acts, obs_out=f32, obs_dtype=torch.float16)
    with pytest.raises(TypeError):
        env.step_obs(acts, obs_out=bf)
    from marl_gpu.rollout import MappoRollout
    with pytest.raises(TypeError):
        MappoRollout(env, 4, obs_dtype=torch.float64)
    # the C entries: an unknown dtype fails with a message and launches nothing
    before = {k: v.clone() for k, v in bf.items()}
    stream = _lib.stream_handle(env.device)
    ptrs = [bf[k].data_ptr() for k in OBS_KEYS]
    assert _lib.lib().mdl_build_obs_as(env._h, 0, E, 7, *ptrs, stream) != 0
    assert b"dtype 7" in _lib.lib().mdl_last_error()
    assert _lib.lib().mdl_step_obs_as(env._h, acts.data_ptr(), 0, 1, None, None, None, 7, *ptrs, stream) != 0
    assert b"dtype 7" in _lib.lib().mdl_last_error()
    torch.cuda.synchronize()
    assert int(env.read_state()["t"].max()) == 0   # the refused step did not run
    for k in OBS_KEYS:
        assert torch.equal(bf[k].view(torch.int16), before[k].view(torch.int16))
    # MDL_OBS_F32 through the _as entry is mdl_build_obs
    a, b = env.build_obs(), env.obs_buffers()
    assert _lib.lib().mdl_build_obs_as(env._h, 0, E, 0, *[b[k].data_ptr() for k in OBS_KEYS], stream) == 0
    for k in OBS_KEYS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    env.close()
