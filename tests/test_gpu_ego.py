"""Robot-centred actor-map windows (BatchedEnv.build_obs_ego, k_ego_maps) against the CPU oracle, bit for
bit: every comparison is with ego_ref.ego_from_full of the ORACLE's actor_map -- never with the engine's
own full-map builder.  Each case (ego_ref.CASES; their input conditions are asserted on the oracle in
test_ego_cpu.py) runs E <= 8 envs for 25 steps with auto-resets and is compared after reset, every third
step and around every auto-reset, at each of its radii, as float32 and as both half types; once per case
and radius a sub-range is written into guard-filled buffers carved at every element offset past a 16-B
line.  MappoRollout(ego_radius=) is held to a float32 twin without a radius."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ego_ref as G  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402

HALF = (torch.float16, torch.bfloat16)
ONE = {torch.float16: 0x3C00, torch.bfloat16: 0x3F80}
SENTINEL = -7.25   # no map element equals it
GUARD = 8          # guard elements on both sides (a multiple of 8: the lead alone sets the offset)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


def make_env(case):
    import marl_gpu
    g = G.grids(case)
    return marl_gpu.BatchedEnv(g if len(g) > 1 else g[0], case.E, case.A, case.P, case.T, seed=case.seed,
                               env_map=case.env_map, tracker=case.tracker, shaping="mappo", max_packages_obs=5,
                               max_robots_state=4, max_packages_state=4)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def want_bits(want, dtype):
    """The oracle's float32 window as the bit patterns of `dtype` (its values are 0 and 1 only)."""
    assert set(np.unique(want)) <= {0.0, 1.0}
    if dtype == torch.float32:
        return want.view(np.uint32)
    return (want.astype(np.uint16) * np.uint16(ONE[dtype]))


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at (env, robot, channel, "
                             f"row, col) {i}: engine {int(got[i]):#x} oracle {int(want[i]):#x}")


def windows(full, R):
    return np.stack([G.ego_from_full(f, R) for f in full])   # [E, A, 6, K, K]


def offset_build(env, R, b0, n, want, dtype, lead, what):
    """build_obs_ego of envs [b0, b0 + n) into a tensor that starts `lead` elements past a 16-B line,
    sentinel guard elements on both sides."""
    cnt = want.size
    buf = torch.full((GUARD + lead + cnt + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + lead:GUARD + lead + cnt].view(want.shape)
    assert out.data_ptr() % 16 == (lead * buf.element_size()) % 16
    got = env.build_obs_ego(R, env_begin=b0, n=n, out=out, dtype=dtype)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    same(bits(out), want_bits(want, dtype), what)
    guard = torch.full((1,), SENTINEL, dtype=dtype)
    r = buf.cpu()
    assert bool((r[:GUARD + lead] == guard).all()) and bool((r[GUARD + lead + cnt:] == guard).all()), \
        f"{what}: a guard element was overwritten"


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_windows_vs_oracle(case):
    env = make_env(case)
    E = case.E
    pts = G.build_points(case)
    sub_at = next(k for k in pts if k > case.T)   # past the first auto-reset
    resets = 0
    try:
        env.reset()
        for k, ints, dn, full in G.trace(case):
            if ints is not None:
                _, _, d = env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
                assert (d.cpu().numpy().astype(bool) == dn).all(), f"step {k}: done"
                resets += int(dn.sum())
            if full is None:
                continue
            for R in case.radii:
                want = windows(full, R)
                what = f"{case.id} step {k} R={R}"
                got = env.build_obs_ego(R)
                assert tuple(got.shape) == (E, case.A, 6, 2 * R + 1, 2 * R + 1) and got.dtype == torch.float32
                same(bits(got), want.view(np.uint32), what)
                for dt in HALF:
                    h = env.build_obs_ego(R, dtype=dt)
                    assert h.dtype == dt
                    same(bits(h), want_bits(want, dt), f"{what} as {dt}")
                    assert torch.equal(h, got.to(dt)), f"{what}: {dt} is not .to() of the float32 result"
                if k != sub_at:
                    continue
                # a sub-range (for the mixed-map cases it crosses both shape boundaries) into a full
                # tensor: the rows before and after it stay untouched
                b0, n = 1, E - 2
                for dt in (torch.float32,) + HALF:
                    whole = torch.full(want.shape, SENTINEL, dtype=dt, device="cuda")
                    env.build_obs_ego(R, env_begin=b0, n=n, out=whole[b0:b0 + n], dtype=dt)
                    same(bits(whole[b0:b0 + n]), want_bits(want[b0:b0 + n], dt), f"{what} envs [1, {E - 1}) as {dt}")
                    rest = torch.cat([whole[:b0], whole[b0 + n:]]).cpu()
                    assert bool((rest == torch.full((1,), SENTINEL, dtype=dt)).all()), f"{what}: a row outside"
                    for lead in range(16 // whole.element_size()):
                        offset_build(env, R, b0, n, want[b0:b0 + n], dt, lead,
                                     f"{what} envs [1, {E - 1}) as {dt}, {lead} past a line")
                # one env, and the last env alone
                same(bits(env.build_obs_ego(R, env_begin=E - 1)), want[E - 1:].view(np.uint32), f"{what} last env")
        assert resets >= E
    finally:
        env.close()


def test_bad_arguments_raise():
    import marl_gpu
    from marl_gpu import _lib
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 4, 3, 8, 10, seed=1)
    try:
        env.reset()
        for R in (0, 16, -2):
            with pytest.raises(ValueError):
                env.build_obs_ego(R)
            with pytest.raises(ValueError):
                env.ego_buffers(R)
        with pytest.raises(TypeError):
            env.build_obs_ego(2, out=env.ego_buffers(2, dtype=torch.float16))   # float32 asked, half given
        with pytest.raises(TypeError):
            env.build_obs_ego(2, out=env.ego_buffers(2), dtype=torch.bfloat16)
        with pytest.raises(TypeError):
            env.build_obs_ego(2, dtype=torch.float64)
        with pytest.raises(ValueError):
            env.build_obs_ego(2, out=env.ego_buffers(2, n=3))                  # too short
        with pytest.raises(ValueError):
            env.build_obs_ego(2, out=env.ego_buffers(2).cpu())
        with pytest.raises(IndexError):
            env.build_obs_ego(2, env_begin=2, n=3)
        assert tuple(env.build_obs_ego(2, env_begin=4).shape) == (0, 3, 6, 5, 5)
        # the C entry: a status and mdl_last_error
        L = _lib.lib()
        out = env.ego_buffers(2)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for args, word in (((0, 4, 0, 0), "radius"), ((0, 4, 16, 0), "radius"), ((0, 4, 2, 3), "dtype"),
                           ((1, 4, 2, 0), "range"), ((-1, 2, 2, 0), "range")):
            assert L.mdl_build_obs_ego(env._h, *args, out.data_ptr(), s) != 0, args
            assert word in L.mdl_last_error().decode(), (args, L.mdl_last_error())
        assert L.mdl_build_obs_ego(env._h, 0, 4, 2, 0, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
    finally:
        env.close()


def test_build_is_capturable():
    """No host round trip: ten calls captured as one hipGraph replay to the eager result."""
    import marl_gpu
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 6, 5, 20, 10, seed=3)
    try:
        env.reset()
        outs = [env.ego_buffers(2) for _ in range(10)]
        want = env.build_obs_ego(2).clone()
        from marl_gpu._capture import capture
        g, _ = capture(env.device, lambda: [env.build_obs_ego(2, out=o) for o in outs])
        for o in outs:
            o.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, want)
    finally:
        env.close()


def test_mappo_rollout_with_windows_against_a_full_map_twin():
    """MappoRollout(ego_radius=2) and a float32 twin without a radius on the same seeds: the window buffer
    is ego_from_full of the twin's full maps, every other buffer is identical, and collect(graph=True)
    is bitwise the eager result."""
    import marl_gpu
    from marl_gpu import rollout as R
    g = grid("map1.txt")
    E, A, P, T, steps = 8, 5, 20, 10, 6

    def make():
        env = marl_gpu.BatchedEnv(g, E, A, P, T, seed=7, tracker="mappo", shaping="mappo", max_other_robots=A - 1,
                                  max_packages_obs=5)
        env.reset()
        return env

    gen = torch.Generator(device="cuda").manual_seed(3)
    envs = [make() for _ in range(3)]
    wa = torch.randn(envs[0].actor_vec_dim, 15, device="cuda", generator=gen)
    wc = torch.randn(envs[0].critic_vec_dim, device="cuda", generator=gen) * 0.01

    def actor(obs, vec):   # reads the map tensor where the full map and its window agree: channel 1 sums to 1
        return vec @ wa + obs[:, 1].sum(dim=(1, 2)).unsqueeze(1) * 0.01

    def critic(gmap, gvec):
        return gvec @ wc

    try:
        twin = R.MappoRollout(envs[0], steps, seed=5)
        ego = R.MappoRollout(envs[1], steps, seed=5, ego_radius=2)
        graphed = R.MappoRollout(envs[2], steps, seed=5, ego_radius=2)
        assert tuple(ego.mb_obs.shape) == (steps, E, A, 6, 5, 5) and tuple(ego.next_obs["actor_map"].shape) == (E, A, 6, 5, 5)
        assert tuple(twin.mb_obs.shape) == (steps, E, A, 6, 10, 10)
        for k in range(3):   # call 0 of `graphed` runs eagerly and captures, calls 1 and 2 replay
            a = [x.clone() for x in twin.collect(actor, critic)]
            b = [x.clone() for x in ego.collect(actor, critic)]
            c = [x.clone() for x in graphed.collect(actor, critic, graph=True)]
            torch.cuda.synchronize()
            want = G.ego_from_full(twin.mb_obs.cpu().numpy(), 2)
            same(bits(ego.mb_obs), want.view(np.uint32).reshape(ego.mb_obs.shape), f"rollout {k}: mb_obs")
            assert torch.equal(b[0], ego.mb_obs.reshape(-1, 6, 5, 5))
            same(bits(ego.next_obs["actor_map"]),
                 G.ego_from_full(twin.next_obs["actor_map"].cpu().numpy(), 2).view(np.uint32), f"rollout {k}: next_obs")
            for i in range(1, len(a)):
                assert torch.equal(a[i], b[i]), f"rollout {k}, output {i}"
            for name in ("mb_vector_obs", "mb_global_states", "mb_global_vector", "mb_actions", "mb_log_probs",
                         "mb_rewards", "mb_dones", "mb_values"):
                assert torch.equal(getattr(twin, name), getattr(ego, name)), f"rollout {k}: {name}"
            for key in ("actor_vec", "critic_map", "critic_vec"):
                assert torch.equal(twin.next_obs[key], ego.next_obs[key]), f"rollout {k}: next_obs[{key}]"
            for i, (x, y) in enumerate(zip(b, c)):
                assert torch.equal(x, y), f"rollout {k}, graphed output {i}"
            assert torch.equal(ego.mb_obs, graphed.mb_obs)
        assert graphed.captured_graphs() == {None: steps}
        s0, s1, s2 = (e.read_state() for e in envs)
        for key in s0:
            assert torch.equal(s0[key], s1[key]) and torch.equal(s0[key], s2[key]), key
        # with obs_dtype the window buffers have that type: its first slot is the float32 rollout's first
        # slot converted (the same seeds and reset state; later slots follow other actions, the vectors
        # being rounded), and every later slot holds 0 / 1.0 with the robot at the centre
        envs.append(make())
        fresh = R.MappoRollout(envs[-1], steps, seed=5, ego_radius=2)
        envs.append(make())
        half = R.MappoRollout(envs[-1], steps, seed=5, ego_radius=2, obs_dtype=torch.bfloat16)
        assert half.mb_obs.dtype == torch.bfloat16 and half.next_obs["actor_map"].dtype == torch.bfloat16
        assert tuple(half.mb_obs.shape) == (steps, E, A, 6, 5, 5)
        fresh.collect(actor, critic)
        half.collect(lambda obs, vec: actor(obs.float(), vec.float()), lambda gm, gv: critic(gm, gv.float()))
        torch.cuda.synchronize()
        assert torch.equal(half.mb_obs[0], fresh.mb_obs[0].to(torch.bfloat16))
        for t in (half.mb_obs, half.next_obs["actor_map"]):
            assert set(np.unique(bits(t))) == {0, ONE[torch.bfloat16]}
            assert bool((t[..., 1, :, :].float().sum(dim=(-1, -2)) == 1).all()) and bool((t[..., 1, 2, 2] == 1).all())
    finally:
        for e in envs:
            e.close()
