"""The critic map on a fixed canvas (BatchedEnv.build_obs_canvas, k_canvas_maps) against the CPU oracle, bit
for bit: the canvas is canvas_ref.canvas_from_full of the ORACLE's critic_map, the vectors are the oracle's
own -- never the engine's builders', except where the identity with build_obs is the thing tested.  Each case
(canvas_ref.CASES; their input conditions are asserted on the oracle in test_canvas_cpu.py) is compared after
reset, every third step and around every auto-reset, as float32 and as both half types; once per case a
sub-range is written into guard-filled buffers carved 1, 2 and 3 floats past a 16-B line.  Masks leave
unmarked rows' sentinels untouched in all three tensors, over the whole range and over [1, E - 1)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import canvas_ref as V  # noqa: E402
import oracle as O  # noqa: E402
from ego_masked_ref import SENTINEL_BITS  # noqa: E402
from golden_io import grid  # noqa: E402

HALF = (torch.float16, torch.bfloat16)
DTYPES = (torch.float32,) + HALF
INT_OF = {4: torch.int32, 2: torch.int16}
GUARD = 8


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


def make_env(case, shaping="mappo"):
    import marl_gpu
    g = V.grids(case)
    return marl_gpu.BatchedEnv(g if len(g) > 1 else g[0], case.E, case.A, case.P, case.T, seed=case.seed,
                               env_map=case.env_map, tracker=case.tracker, shaping=shaping, max_packages_obs=V.MP,
                               max_robots_state=V.MR, max_packages_state=V.MPS)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def want_bits(want, dtype):
    """The oracle's float32 array as the bit patterns of `dtype`: the float32 value rounded once."""
    want = np.ascontiguousarray(want, np.float32)
    if dtype == torch.float32:
        return want.view(np.uint32)
    return bits(torch.from_numpy(want).to(dtype))


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {i}: engine "
                             f"{int(got[i]):#x} oracle {int(want[i]):#x}")


def sentinel(shape, dtype):
    es = torch.empty((), dtype=dtype).element_size()
    v = SENTINEL_BITS[es]
    v = v - (1 << 8 * es) if v >= 1 << (8 * es - 1) else v
    return torch.full(shape, v, dtype=INT_OF[es], device="cuda").view(dtype)


def sentinel_bits(dtype):
    return SENTINEL_BITS[4 if dtype == torch.float32 else 2]


def check_all(got, want, dtype, what, sl=slice(None)):
    for k in V.KEYS:
        assert got[k].dtype == dtype
        same(bits(got[k]), want_bits(want[k][sl], dtype), f"{what}: {k} as {dtype}")


def offset_build(env, canvas, b0, n, want, lead, what):
    """build_obs_canvas of envs [b0, b0 + n) into float32 tensors that start `lead` floats past a 16-B line,
    sentinel guard elements on both sides."""
    out, bufs = {}, {}
    for k in V.KEYS:
        cnt = want[k][b0:b0 + n].size
        buf = sentinel((GUARD + lead + cnt + GUARD,), torch.float32)
        assert buf.data_ptr() % 16 == 0
        out[k] = buf[GUARD + lead:GUARD + lead + cnt].view(want[k][b0:b0 + n].shape)
        assert out[k].data_ptr() % 16 == 4 * lead
        bufs[k] = buf
    got = env.build_obs_canvas(canvas, env_begin=b0, n=n, out=out)
    torch.cuda.synchronize()
    for k in V.KEYS:
        assert got[k].data_ptr() == out[k].data_ptr()
        same(bits(out[k]), want_bits(want[k][b0:b0 + n], torch.float32), f"{what}: {k}")
        r = bits(bufs[k])
        cnt = out[k].numel()
        assert (r[:GUARD + lead] == SENTINEL_BITS[4]).all() and (r[GUARD + lead + cnt:] == SENTINEL_BITS[4]).all(), \
            f"{what}: a guard element of {k} was overwritten"


@pytest.mark.parametrize("case", V.CASES, ids=[c.id for c in V.CASES])
def test_canvas_and_vectors_vs_oracle(case):
    env = make_env(case)
    E, canvas = case.E, case.canvas
    sh = V.shapes(case)
    pts = V.build_points(case)
    sub_at = next((k for k in pts if k > case.T), pts[-1])   # past the first auto-reset where the case has one
    resets = 0
    try:
        env.reset()
        for k, ints, dn, obs in V.trace(V.base(case)):
            if ints is not None:
                _, _, d = env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
                assert (d.cpu().numpy().astype(bool) == dn).all(), f"step {k}: done"
                resets += int(dn.sum())
            if obs is None:
                continue
            want = V.want(obs, canvas)
            what = f"{case.id} step {k}"
            got = env.build_obs_canvas(canvas)
            assert tuple(got["critic_map"].shape) == (E, 4) + canvas
            check_all(got, want, torch.float32, what)
            for dt in HALF:
                h = env.build_obs_canvas(canvas, dtype=dt)
                check_all(h, want, dt, what)
                for key in V.KEYS:
                    assert torch.equal(h[key], got[key].to(dt)), f"{what}: {key} as {dt} is not .to() of float32"
            # identity: where the canvas is a group's own map shape it is build_obs's critic_map, byte for
            # byte; on a single-shape engine the vectors are build_obs's too
            b = 0
            while b < E:
                e1 = next((e for e in range(b, E) if sh[e] != sh[b]), E)
                if sh[b] == canvas:
                    full = env.build_obs(env_begin=b, n=e1 - b, which=("actor_vec", "critic_map", "critic_vec"))
                    assert bits(got["critic_map"][b:e1]).tobytes() == bits(full["critic_map"]).tobytes(), what
                    for key in ("actor_vec", "critic_vec"):
                        assert torch.equal(got[key][b:e1], full[key]), f"{what}: {key} of envs [{b}, {e1})"
                b = e1
            if k != sub_at or E < 3:
                continue
            # a sub-range (for the mixed cases it crosses both shape boundaries: the rows are indexed by
            # w, the maps by e) into whole tensors: the rows before and after it stay untouched
            b0, n = 1, E - 2
            for dt in DTYPES:
                whole = {key: sentinel(want[key].shape, dt) for key in V.KEYS}
                env.build_obs_canvas(canvas, env_begin=b0, n=n, out={key: v[b0:b0 + n] for key, v in whole.items()},
                                     dtype=dt)
                for key in V.KEYS:
                    same(bits(whole[key][b0:b0 + n]), want_bits(want[key][b0:b0 + n], dt),
                         f"{what} envs [1, {E - 1}): {key} as {dt}")
                    rest = bits(torch.cat([whole[key][:b0], whole[key][b0 + n:]]))
                    assert (rest == sentinel_bits(dt)).all(), f"{what}: a row of {key} outside the range"
            for lead in (1, 2, 3):
                offset_build(env, canvas, b0, n, want, lead, f"{what} envs [1, {E - 1}), {lead} floats past a line")
            # the last env alone, and each output on its own
            last = env.build_obs_canvas(canvas, env_begin=E - 1)
            check_all(last, want, torch.float32, f"{what} last env", slice(E - 1, E))
            for key in V.KEYS:
                only = {kk: sentinel(want[kk].shape, torch.float32) for kk in V.KEYS}
                env.build_obs_canvas(canvas, out=only, which=(key,))
                for kk in V.KEYS:
                    if kk == key:
                        same(bits(only[kk]), want_bits(want[kk], torch.float32), f"{what}: which=({key},)")
                    else:
                        assert (bits(only[kk]) == SENTINEL_BITS[4]).all(), f"{what}: which=({key},) wrote {kk}"
        assert resets >= (E if case.steps > case.T else 0)
    finally:
        env.close()


def masks_of(case):
    E = case.E
    sh = V.shapes(case)
    m = {"all": np.ones(E, np.uint8), "none": np.zeros(E, np.uint8)}
    m["env0"] = np.zeros(E, np.uint8)
    m["env0"][0] = 1
    m["odd"] = (np.arange(E) % 2 == 1).astype(np.uint8) * np.array([1, 0x80, 0xFF, 2], np.uint8)[np.arange(E) % 4]
    m["one_per_group"] = np.zeros(E, np.uint8)
    for e in range(E):
        if e == 0 or sh[e] != sh[e - 1]:
            m["one_per_group"][min(e + 1, E - 1) if e else 0] = 1   # the first group's env 0, the others' second
    return m


def run_masks(env, case, want, ranges, masks, dtypes, what):
    E, canvas = case.E, case.canvas
    for name, m in masks.items():
        rows = torch.from_numpy(m).cuda()
        for b0, n in ranges:
            for dt in dtypes:
                out = {k: sentinel(want[k][b0:b0 + n].shape, dt) for k in V.KEYS}
                env.build_obs_canvas(canvas, env_begin=b0, n=n, rows=rows, out=out, dtype=dt)
                torch.cuda.synchronize()
                for k in V.KEYS:
                    exp = want_bits(want[k][b0:b0 + n], dt).copy()
                    exp[m[b0:b0 + n] == 0] = sentinel_bits(dt)
                    same(bits(out[k]), exp, f"{what} mask {name} envs [{b0}, {b0 + n}): {k} as {dt}")


@pytest.mark.parametrize("cid", ["m1_pad_stale", "mixed_stale", "mixed_stale_odd", "mixed_fresh_odd", "lines"])
def test_masks_leave_unmarked_rows_untouched(cid):
    """Sentinel-filled outputs under every mask, over the whole range and over [1, E - 1): the sub-range is
    where a mask read by output row (the canvas kernel's, or the vector runs handed `rows` and not
    `rows + b`) marks other rows."""
    case = V.BY_ID[cid]
    env = make_env(case)
    E = case.E
    try:
        env.reset()
        d = V.Driver(V.base(case))
        for _ in range(case.T + 3):   # past the auto-reset
            ints = d.actions()
            d.step(ints)
            env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
        want = V.want(d.obs_all(), case.canvas)
        masks = masks_of(case)
        for b0, n in ((1, E - 2),):   # the sub-range shifts every mask but the constant ones
            assert sum(not np.array_equal(m[b0:b0 + n] != 0, m[:n] != 0) for m in masks.values()) >= 3
        run_masks(env, case, want, ((0, E), (1, E - 2)), masks, DTYPES, cid)
        # a fresh tensor (out=None) under a mask starts as zeros
        got = env.build_obs_canvas(case.canvas, rows=torch.from_numpy(masks["env0"]).cuda())
        for k in V.KEYS:
            assert not bool(got[k][1:].any()), k
            same(bits(got[k][:1]), want_bits(want[k][:1], torch.float32), f"{cid}: fresh {k}")
    finally:
        env.close()


def test_67_envs_with_a_mask_over_a_sub_range():
    case = V.BY_ID["e67"]
    env = make_env(case)
    try:
        env.reset()
        tr = V.trace(V.base(case))
        for k, ints, dn, obs in tr:
            if ints is not None:
                env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
        want = V.want(tr[-1][3], case.canvas)
        m3 = (np.arange(case.E) % 3 == 0).astype(np.uint8)
        but33 = np.ones(case.E, np.uint8)
        but33[33] = 0
        run_masks(env, case, want, ((5, 59),), {"third": m3, "but33": but33}, (torch.float32, torch.float16), "e67")
    finally:
        env.close()


def test_refusals_leave_the_engine_usable():
    import marl_gpu
    from marl_gpu import _lib
    case = V.BY_ID["mixed_fresh"]
    env = make_env(case)
    E, A = case.E, case.A
    try:
        env.reset()
        ok = env.build_obs_canvas((20, 20))
        torch.cuda.synchronize()
        with pytest.raises(_lib.MdlError, match="smaller than the 20 x 20 map of env 3"):
            env.build_obs_canvas((19, 25))                     # a map of the range is taller
        with pytest.raises(_lib.MdlError, match="smaller than"):
            env.build_obs_canvas((25, 19))                     # ... wider
        with pytest.raises(_lib.MdlError, match="smaller than"):
            env.build_obs_canvas((10, 10), env_begin=2, n=3)   # envs 3, 4 are 20 x 20
        small = env.build_obs_canvas((10, 10), env_begin=0, n=3)   # the 10 x 10 group alone fits
        assert torch.equal(small["critic_map"], ok["critic_map"][:3, :, :10, :10])
        assert torch.equal(env.build_obs_canvas((7, 9), env_begin=5)["critic_map"][..., :7],
                           ok["critic_map"][5:, :, :7, :7])
        for bad in ((129, 128), (20, 256), (256, 20), (0, 20), (20, 0), (20,), 20, (20.0, 20), (True, 20)):
            with pytest.raises(ValueError):
                env.build_obs_canvas(bad)
            with pytest.raises(ValueError):
                env.canvas_buffers(bad)
        with pytest.raises(TypeError):
            env.build_obs_canvas((20, 20), dtype=torch.float64)
        with pytest.raises(TypeError):
            env.build_obs_canvas((20, 20), out=env.canvas_buffers((20, 20), dtype=torch.float16))
        with pytest.raises(TypeError):
            env.build_obs_canvas((20, 20), out=env.canvas_buffers((20, 20)), dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            env.build_obs_canvas((21, 23), out=env.canvas_buffers((20, 20)))    # too short for the canvas
        with pytest.raises(ValueError):
            env.build_obs_canvas((20, 20), out=env.canvas_buffers((20, 20), n=E - 1))
        with pytest.raises(KeyError):
            env.build_obs_canvas((20, 20), out=dict(critic_map=ok["critic_map"]))   # a named entry is missing
        with pytest.raises(IndexError):
            env.build_obs_canvas((20, 20), env_begin=2, n=E)
        with pytest.raises(TypeError):
            env.build_obs_canvas((20, 20), rows=torch.ones(E, dtype=torch.bool, device="cuda"))
        with pytest.raises(ValueError):
            env.build_obs_canvas((20, 20), rows=torch.ones(E - 1, dtype=torch.uint8, device="cuda"))
        assert tuple(env.build_obs_canvas((20, 20), env_begin=E)["critic_map"].shape) == (0, 4, 20, 20)
        # the C entry: a status and mdl_last_error
        L = _lib.lib()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        o = env.canvas_buffers((128, 128))
        ptrs = (o["actor_vec"].data_ptr(), o["critic_map"].data_ptr(), o["critic_vec"].data_ptr())
        for args, word in (((0, E, None, 0, 129, 128), "Hc*Wc"), ((0, E, None, 0, 20, 256), "[1,255]"),
                           ((0, E, None, 0, 0, 20), "[1,255]"), ((0, E, None, 3, 20, 20), "dtype"),
                           ((0, E, None, -1, 20, 20), "dtype"), ((1, E, None, 0, 20, 20), "range"),
                           ((-1, 2, None, 0, 20, 20), "range"), ((0, E, None, 0, 19, 20), "smaller than")):
            assert L.mdl_build_obs_canvas(env._h, *args, *ptrs, s) != 0, args
            assert word in L.mdl_last_error().decode(), (args, L.mdl_last_error())
        assert L.mdl_build_obs_canvas(env._h, 0, E, None, 0, 20, 20, None, None, None, s) == 0   # nothing to write
        assert L.mdl_build_obs_canvas(env._h, 0, E, None, 0, 128, 128, *ptrs, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(o["critic_map"][..., :20, :20], ok["critic_map"])
        # step_episode with an observation on a mixed engine: today's refusal, from Python and from C
        active = torch.ones(E, dtype=torch.uint8, device="cuda")
        acts = torch.zeros((E, A), dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="mix map shapes"):
            env.step_episode(acts, active)
        with pytest.raises(ValueError, match="mix map shapes"):
            env.step_episode(acts, active, which=("critic_vec",))
        rc = L.mdl_step_episode(env._h, acts.data_ptr(), 0, active.data_ptr(), None, None, None, None, None, None,
                                None, o["critic_vec"].data_ptr(), s)
        assert rc != 0 and "mdl_step_episode: the envs mix map shapes (same-shape run ends at 3)" in \
            L.mdl_last_error().decode()
        # ... and the engine still builds what it built before
        again = env.build_obs_canvas((20, 20))
        for k in V.KEYS:
            assert torch.equal(again[k], ok[k]), k
    finally:
        env.close()


def test_build_is_capturable():
    """No host round trip: masked and unmasked calls captured as one hipGraph replay to the eager result."""
    from marl_gpu._capture import capture
    case = V.BY_ID["mixed_stale_odd"]
    env = make_env(case)
    try:
        env.reset()
        rows = torch.from_numpy(masks_of(case)["odd"]).cuda()
        want = {k: v.clone() for k, v in env.build_obs_canvas(case.canvas).items()}
        outs = [{k: sentinel(v.shape, torch.float32) for k, v in want.items()} for _ in range(4)]

        def run():
            for i, o in enumerate(outs):
                env.build_obs_canvas(case.canvas, rows=rows if i % 2 else None, out=o)
        g, _ = capture(env.device, run)
        for o in outs:
            for k in o:
                o[k].copy_(sentinel(o[k].shape, torch.float32))
        g.replay()
        torch.cuda.synchronize()
        keep = torch.from_numpy(masks_of(case)["odd"] != 0)
        for i, o in enumerate(outs):
            for k in V.KEYS:
                if i % 2:
                    assert bits(o[k][keep]).tobytes() == bits(want[k][keep]).tobytes()
                    assert (bits(o[k][~keep]) == SENTINEL_BITS[4]).all()
                else:
                    assert bits(o[k]).tobytes() == bits(want[k]).tobytes()
    finally:
        env.close()


def test_step_episode_without_observations_on_a_mixed_engine():
    """step_episode(which=()) on mixed_fresh, hand-driven with a mask: rewards, done, filled, active and the
    whole state against the oracle stepped without reset; the unmarked envs' state is unchanged."""
    case = V.BY_ID["mixed_fresh"]
    env = make_env(case, shaping="qmix")
    E, A = case.E, case.A
    try:
        env.reset()
        ref = V.Replay(V.base(case), consts=O.QMIX_CONSTS, auto_reset=False)
        running = np.array([1, 0, 1, 1, 0, 1, 1, 1], bool)
        active = torch.from_numpy(running.astype(np.uint8) * np.uint8(0x81)).cuda()   # non-zero = set
        filled = torch.full((E,), 0xA5, dtype=torch.uint8, device="cuda")
        rs = np.random.RandomState(11)
        ended = 0

        def check_state(what):
            s = env.read_state()
            torch.cuda.synchronize()
            s = {k: v.cpu().numpy() for k, v in s.items()}
            for e in range(E):
                st = ref.d.state(e)
                assert np.array_equal(s["robots"][e], st["robots"]), f"{what}: robots of env {e}"
                assert np.array_equal(s["pkgs"][e], st["pkgs"]), f"{what}: packages of env {e}"
                assert s["t"][e] == st["t"], f"{what}: t of env {e}"
                assert s["total_reward"][e].tobytes() == np.float64(st["total_reward"]).tobytes(), what
                assert np.array_equal(env.tracker_rows(s, e), ref.d.b[e].tracker(0).rows()), f"{what}: tracker {e}"

        check_state("after reset")
        for k in range(case.T + 1):
            ints = rs.randint(0, 15, size=(E, A)).astype(np.uint8)
            r, sh, dn, obs = env.step_episode(torch.from_numpy(ints).cuda(), active, filled=filled, which=())
            assert all(v is None for v in obs.values())
            r0, sh0, dn0 = ref.step(ints, running)
            what = f"step {k}"
            assert r.cpu().numpy().tobytes() == r0.tobytes(), f"{what}: r_env"
            assert sh.cpu().numpy().tobytes() == sh0.tobytes(), f"{what}: r_shaped"
            assert np.array_equal(dn.cpu().numpy().astype(bool), dn0), f"{what}: done"
            assert np.array_equal(filled.cpu().numpy(), running.astype(np.uint8)), f"{what}: filled"
            ended += int(dn0.sum())
            running = running & ~dn0
            assert np.array_equal(active.cpu().numpy() != 0, running), f"{what}: active"
            if k % 3 == 0 or not running.any():
                check_state(what)
        assert ended == 6 and not running.any()
        check_state("at the end")   # envs 1 and 4 never moved: the oracle's are at their reset state
    finally:
        env.close()
