"""Every observation-builder instantiation (tests/obs_matrix.py: 18 symbols) against the CPU oracle at
the edges of the builders' run-time layout decisions, bit for bit on the uint32 / uint16 patterns --
never builder against builder.

Each case first asserts, on the oracle's trace alone, that its inputs exercise what it is there for
(obs_ref.check_inputs), then that the engine names the expected kernel (obs_kernel_name, which comes
from the selection the launch itself runs) for float32, float16 and bfloat16.  Then, along 2T+3 steps
with two auto-resets (the K cases: as obs_matrix states), at every build point: build_obs of every env,
each tensor alone through which=, and both half types against obs_dtype_ref.round_to(oracle); once per
case the sub-range [1, n-1) of every map group into buffers whose tensors start 1, 2 and 3 elements
past a 16-B line between guard elements; and, where the engine fuses step and observations, step_obs on
a second engine after every step.  test_step_episode_masked_rows drives step_episode under a mask."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import obs_matrix as M  # noqa: E402
import obs_ref as R  # noqa: E402
import oracle as O  # noqa: E402
from obs_dtype_ref import HALF_DTYPES, bits16, round_to  # noqa: E402

OBS_KEYS = R.OBS_KEYS
SENTINEL = -7.25   # no observation feature equals it
GUARD = 8          # guard elements in front of an offset tensor (a multiple of four: the lead sets the offset)
EPISODE_CUTS = {1: 3, 3: 7, 0: 12}   # env -> the step its episode is cut at by the caller (step_matrix's pattern)
EPISODE_ZERO_MASK_STEP = 4           # one extra call with an all-zero mask before this step


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


def make_env(case):
    import marl_gpu
    g = R.grids(case)
    return marl_gpu.BatchedEnv(g if len(g) > 1 else g[0], case.E, case.A, case.P, case.T, seed=case.seed,
                               env_map=case.env_map, tracker=case.tracker, shaping="mappo",
                               max_other_robots=case.MO, max_packages_obs=case.MP, max_robots_state=case.MR,
                               max_packages_state=case.MPs, obs_max_time_steps=case.obsT, obs_builder=case.builder)


def same_bits(got, want, what):
    """Two arrays of bit patterns (uint32 / uint16) must be equal; a difference only in the sign of a
    zero is reported with the side that produced the negative one."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    bad = np.argwhere(got != want)
    top = np.array(1 << (8 * got.itemsize - 1), got.dtype)
    i = tuple(bad[0])
    zeros = [(int(got[tuple(j)]), int(want[tuple(j)])) for j in bad
             if (got[tuple(j)] | top) == top and (want[tuple(j)] | top) == top]
    note = ""
    if zeros:
        side = "engine" if zeros[0][0] == int(top) else "oracle"
        note = f"; {len(zeros)} differ only in the sign of zero (-0 from the {side})"
    raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {i}: "
                         f"engine {int(got[i]):#x} oracle {int(want[i]):#x}{note}")


def f32_bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def check_f32(obs, want, what, keys=OBS_KEYS):
    for k in keys:
        same_bits(f32_bits(obs[k]), want[k].view(np.uint32), f"{what}: {k}")


def check_half(obs, want, dtype, what):
    for k in OBS_KEYS:
        same_bits(bits16(obs[k]), round_to(want[k], dtype), f"{what}: {k} as {dtype}")


def check_out(r, sh, dn, want, what):
    same_bits(r.cpu().numpy().view(np.uint64), want[0].view(np.uint64), f"{what}: r_env")
    same_bits(sh.cpu().numpy().view(np.uint32), want[1].view(np.uint32), f"{what}: r_shaped")
    assert (dn.cpu().numpy().astype(bool) == want[2]).all(), f"{what}: done"


def offset_build(env, b0, n, want, dtype, lead, what):
    """build_obs of envs [b0, b0+n) into tensors that start `lead` elements past a 16-B line, with
    sentinel guard elements on both sides; want: the oracle's rows of those envs."""
    raw, out = {}, {}
    for k in OBS_KEYS:
        shp = (n,) + want[k].shape[1:]
        cnt = int(np.prod(shp))
        buf = torch.full((GUARD + lead + cnt + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        raw[k] = buf
        out[k] = buf[GUARD + lead:GUARD + lead + cnt].view(shp)
        assert (out[k].data_ptr() % 16) == (lead * buf.element_size()) % 16
    env.build_obs(env_begin=b0, n=n, out=out, dtype=dtype)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        check_f32(out, want, what)
    else:
        check_half(out, want, dtype, what)
    guard = torch.full((1,), SENTINEL, dtype=dtype)
    for k in OBS_KEYS:
        r = raw[k].cpu()
        cnt = out[k].numel()
        assert bool((r[:GUARD + lead] == guard).all()) and bool((r[GUARD + lead + cnt:] == guard).all()), \
            f"{what}: {k}: a guard element was overwritten"


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_builders_vs_oracle(case):
    R.check_inputs(case)
    f = R.select(case)
    groups = R.groups(case)
    pts = R.build_points(case)
    sub_at = pts[len(pts) // 2] if case.steps is None else pts[-1]   # past the first reset where there is one
    env = make_env(case)
    fused = R.fused(case)
    env2 = make_env(case) if fused else None
    try:
        assert env.obs_kernel_name() == case.symbol == f["symbol"]
        assert {k: f[k] for k in ("small", "RL", "sw", "one_pass", "gen_sort", "gen_map")} == \
            {k: getattr(case, k) for k in ("small", "RL", "sw", "one_pass", "gen_sort", "gen_map")}
        for dt in HALF_DTYPES:
            name = env.obs_kernel_name(dt)
            assert name == R.half_symbol(case.symbol, str(dt).replace("torch.", "")) and name in M.SYMBOLS
        env.reset()
        if fused:
            env2.reset()
            assert env2.step_kernel_name(with_obs=True).startswith("mdl::k_step_obs<")
        for k, ints, out, obs, is_pt in R.walk(case, every_step_obs=fused):
            a = torch.from_numpy(ints).cuda()
            check_out(*env.step(a, auto_reset=True), out, f"step {k}")
            if fused:
                r, sh, dn, o2 = env2.step_obs(a, auto_reset=True)
                check_out(r, sh, dn, out, f"step_obs {k}")
                check_f32(o2, {key: np.concatenate([g[key] for g in obs]) for key in OBS_KEYS}, f"step_obs {k}")
            if not is_pt:
                continue
            for (b0, n, _), want in zip(groups, obs):
                what = f"step {k}, envs [{b0}, {b0 + n})"
                check_f32(env.build_obs(b0, n), want, what)
                for key in OBS_KEYS:
                    check_f32(env.build_obs(b0, n, which=(key,)), want, f"{what}, which={key}", keys=(key,))
                for dt in HALF_DTYPES:
                    check_half(env.build_obs(b0, n, dtype=dt), want, dt, what)
                if k == sub_at and n >= 3:
                    sub = {key: v[1:n - 1] for key, v in want.items()}
                    for lead in (1, 2, 3):
                        for dt in (torch.float32,) + tuple(HALF_DTYPES):
                            offset_build(env, b0 + 1, n - 2, sub, dt, lead,
                                         f"step {k}, envs [{b0 + 1}, {b0 + n - 1}) {lead} past a line")
    finally:
        env.close()
        if env2 is not None:
            env2.close()


@pytest.mark.parametrize("cid", M.MASKED)
def test_step_episode_masked_rows(cid):
    """step_episode under the step matrix's mask pattern (three episodes cut by the caller, one call with
    an all-zero mask, the rest running to T, never a reset): the written rows equal the oracle's, the
    rows of the envs left out keep the sentinel they were filled with."""
    case = M.BY_ID[cid]
    d = R.Driver(case, singles=True)
    env = make_env(case)
    E = case.E
    sent = np.float32(SENTINEL).view(np.uint32)
    try:
        env.reset()
        obs_out = env.obs_buffers()
        outs = (torch.zeros(E, dtype=torch.float64, device="cuda"), torch.zeros(E, dtype=torch.float32, device="cuda"),
                torch.zeros(E, dtype=torch.uint8, device="cuda"))
        filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
        mask = np.ones(E, bool)
        sizes, zero_calls, written = set(), 0, 0
        for k in range(case.T):
            for e, at in EPISODE_CUTS.items():
                if at == k:
                    mask[e] = False
            done = np.zeros(E, bool)
            for m in ([np.zeros(E, bool)] if k == EPISODE_ZERO_MASK_STEP else []) + [mask.copy()]:
                what = f"step {k} (mask {m.astype(int).tolist()})"
                ints = d.actions(active=m)
                want = d.step(ints, auto_reset=False, active=m)
                rows = d.obs()
                active = torch.from_numpy(m.astype(np.uint8)).cuda()
                for v in obs_out.values():
                    v.fill_(SENTINEL)
                outs[0].fill_(float("nan"))
                outs[1].fill_(float("nan"))
                outs[2].fill_(9)
                filled.fill_(9)
                r, sh, dn, obs = env.step_episode(torch.from_numpy(ints).cuda(), active, out=outs, filled=filled,
                                                  obs_out=obs_out)
                check_out(r, sh, dn, want, what)
                assert (filled.cpu().numpy() == m.astype(np.uint8)).all(), f"{what}: filled"
                assert (active.cpu().numpy().astype(bool) == (m & ~want[2])).all(), f"{what}: the mask after the call"
                for key in OBS_KEYS:
                    x = f32_bits(obs[key])
                    for e in range(E):
                        if m[e]:
                            same_bits(x[e], rows[e][key][0].view(np.uint32), f"{what}: {key} of env {e}")
                            written += 1
                        else:
                            assert (x[e] == sent).all(), f"{what}: {key} row of env {e} (left out) was written"
                sizes.add(int(m.sum()))
                zero_calls += int(not m.any())
                done = want[2]
            mask &= ~done
        # the inputs did what the pattern means: E, E-1, 0, E-2, E-3 envs active, and every episode ended
        assert len(sizes) == len(EPISODE_CUTS) + 2 and zero_calls == 1 and not mask.any() and written > 0
    finally:
        env.close()
