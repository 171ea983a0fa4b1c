"""Robot-centred IDQ / map-QMIX windows on the device (BatchedEnv.build_obs_alt_ego, k_alt_ego) against
alt_ego_ref.alt_ego_from_full of the ORACLE's convert_state, bit for bit (channel 1 holds float32 urgencies),
between guard rows of a NaN-payload sentinel: every case, radius and build point, sub-ranges whose output
starts 1, 2 and 3 floats past a 16-byte line, the row masks (indexed by env id), past one workgroup and one
XCD round, the refusals, and a captured masked call that follows the mask's new contents.  The input
conditions of the cases are pinned on the oracle by test_alt_ego_cpu.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import alt_ego_ref as X  # noqa: E402
import ego_masked_ref as M  # noqa: E402
import ego_ref as G  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402

SENT = np.uint32(M.SENTINEL_BITS[4])   # a quiet NaN with a payload: no urgency, 0.0 or 1.0 has these bits
GUARD = 8                              # floats: the guards keep the 16-byte phase of what lies between them
MASK_CASES = ("m1_a5_stale", "m7_wide_fresh", "s64_a16_fresh", "s64_a64_groups", "mixed_stale")


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def windows(full, R):
    """The oracle's windows of every env as bit patterns [E, A, 6, K, K]."""
    return bits(np.stack([X.alt_ego_from_full(f, R) for f in full]))


def dev_mask(m):
    return torch.from_numpy(np.ascontiguousarray(m, np.uint8)).cuda()


def build_checked(env, R, want, what, b0=0, n=None, lead=0, mask=None):
    """Build envs [b0, b0 + n) at `lead` floats past a 16-byte line between sentinel guards; the rows the
    mask marks (all without one) are the oracle's bit for bit, every other element is the sentinel."""
    n = env.E - b0 if n is None else n
    want = want[b0:b0 + n]
    row = want[0].size
    buf = torch.empty(GUARD + lead + n * row + GUARD, dtype=torch.int32, device="cuda").fill_(int(SENT))
    assert buf.data_ptr() % 16 == 0
    out = buf[GUARD + lead:GUARD + lead + n * row].view(torch.float32).view(want.shape)
    assert out.data_ptr() % 16 == 4 * lead
    got = env.build_obs_alt_ego(R, env_begin=b0, n=n, rows=None if mask is None else dev_mask(mask), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = raw(buf)
    body = host[GUARD + lead:GUARD + lead + n * row].reshape(want.shape)
    assert (host[:GUARD + lead] == SENT).all() and (host[GUARD + lead + n * row:] == SENT).all(), \
        f"{what}: a guard element was overwritten"
    sel = np.ones(n, bool) if mask is None else mask[b0:b0 + n] != 0   # by env id, not by output row
    for i in range(n):
        if not sel[i]:
            assert (body[i] == SENT).all(), f"{what}: env {b0 + i} is unmarked and was written"
        elif body[i].tobytes() != want[i].tobytes():
            bad = np.argwhere(body[i] != want[i])
            a, ch, y, x = bad[0]
            raise AssertionError(f"{what}: env {b0 + i}: {len(bad)} elements differ from the oracle, first at (robot, "
                                 f"channel, row, col) {tuple(bad[0])}: {body[i][a, ch, y, x]:#x} != {want[i][a, ch, y, x]:#x}")
    return body


def sub_ranges(E):
    """(env_begin, n, lead): env_begin > 0, the output 1, 2 and 3 floats past a 16-byte line."""
    return [(b0, max(1, E - b0 - 1), lead) for lead, b0 in ((1, 1), (2, min(2, E - 1)), (3, min(3, E - 1)))]


def run_case(case, at_point):
    env = make_env(case)
    try:
        env.reset()
        for k, ints, dn, full in X.trace(case):
            if ints is not None:
                env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
            if full is not None:
                at_point(env, k, full)
    finally:
        env.close()


# ---------------------------------------------------------------- 1. every case against the oracle
@pytest.mark.parametrize("cid", [c.id for c in X.CASES])
def test_windows_vs_oracle(cid):
    case = X.BY_ID[cid]
    E = case.E
    sub_at = next(k for k in X.build_points(case) if k >= case.T)   # past the first auto-reset (step T - 1)
    seen = dict(points=0, urg=0)

    def at_point(env, k, full):
        seen["points"] += 1
        own = env.build_obs_alt(which=("idq_obs",))["idq_obs"].cpu().numpy() if cid in X.SINGLE_MAP else None
        for R in case.radii:
            want = windows(full, R)
            what = f"{cid} step {k} R={R}"
            got = build_checked(env, R, want, what)
            seen["urg"] += int(((got[:, :, 1] != 0) & (got[:, :, 1] != 0x3F800000)).sum())
            if own is not None:   # the engine's own full tensor, cropped
                assert bits(X.alt_ego_from_full(own, R)).tobytes() == got.tobytes(), f"{what}: crop of build_obs_alt"
            if k == sub_at:   # mixed_*: the first range crosses both map boundaries
                for b0, n, lead in sub_ranges(E):
                    build_checked(env, R, want, f"{what} envs [{b0}, {b0 + n}) lead {lead}", b0, n, lead)

    run_case(case, at_point)
    assert seen["points"] == len(X.build_points(case)) and seen["urg"] > 0   # fractional urgencies came through


# ---------------------------------------------------------------- 2. row masks
@pytest.mark.parametrize("cid", MASK_CASES)
def test_masks_are_indexed_by_env_id(cid):
    case = X.BY_ID[cid]
    E = case.E
    masks = M.mask_patterns(E)
    assert set(masks) == {"none", "all", "first", "last", "even", "odd", "bytes"}
    pts = X.build_points(case)
    at = {pts[1], next(k for k in pts if k >= case.T)}   # early in the first episode, and past the auto-reset

    def at_point(env, k, full):
        if k not in at:
            return
        R = case.radii[-1]
        want = windows(full, R)
        for name, m in masks.items():
            what = f"{cid} step {k} R={R} mask {name}"
            build_checked(env, R, want, what, mask=m)
            b0, n = 1, E - 2   # a mask indexed by output row would build env e under rows[e - 1]
            build_checked(env, R, want, f"{what} envs [{b0}, {b0 + n})", b0, n, lead=1, mask=m)
        if k == pts[1]:   # a fresh tensor under a mask starts as zeros
            m = masks["even"]
            z = raw(env.build_obs_alt_ego(R, rows=dev_mask(m)))
            assert not z[m == 0].any() and z[m != 0].tobytes() == want[m != 0].tobytes()

    run_case(case, at_point)


def test_masks_past_one_workgroup_and_xcd_round():
    case = M.BIG
    masks = dict(M.big_masks(), all=np.ones(case.E, np.uint8))
    n = []

    def at_point(env, k, full):
        want = windows(full, 2)
        build_checked(env, 2, want, f"{case.id} step {k}")
        for name, m in masks.items():
            build_checked(env, 2, want, f"{case.id} step {k} mask {name}", mask=m)
        if k == case.steps - 1:
            for name, m in masks.items():
                build_checked(env, 2, want, f"{case.id} last mask {name}", 5, 59, lead=2, mask=m)
        n.append(k)

    run_case(case, at_point)
    assert len(n) >= 3 and M.blocks(case.E, 4) == (17, 3)


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_engine_usable():
    import marl_gpu
    from marl_gpu import _lib
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 4, 3, 8, 10, seed=1)
    try:
        env.reset()
        ok = torch.ones(4, dtype=torch.uint8, device="cuda")
        want = env.build_obs_alt_ego(2)
        assert tuple(want.shape) == (4, 3, 6, 5, 5) and want.dtype == torch.float32
        full = env.build_obs_alt(which=("idq_obs",))["idq_obs"].cpu().numpy()
        assert raw(want).tobytes() == bits(X.alt_ego_from_full(full, 2)).tobytes()
        for R in (0, 16):
            with pytest.raises(ValueError, match="radius"):
                env.build_obs_alt_ego(R)
        with pytest.raises(TypeError, match="out"):
            env.build_obs_alt_ego(2, out=torch.empty((4, 3, 6, 5, 5), dtype=torch.float16, device="cuda"))
        with pytest.raises(ValueError, match="out"):
            env.build_obs_alt_ego(2, out=torch.empty(4 * 3 * 6 * 25 - 1, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="rows"):
            env.build_obs_alt_ego(2, rows=ok[:3])
        with pytest.raises(TypeError, match="rows"):
            env.build_obs_alt_ego(2, rows=ok.to(torch.int32))
        with pytest.raises(TypeError, match="rows"):
            env.build_obs_alt_ego(2, rows=ok.bool())
        with pytest.raises(IndexError):
            env.build_obs_alt_ego(2, env_begin=2, n=3)
        assert tuple(env.build_obs_alt_ego(2, env_begin=4).shape) == (0, 3, 6, 5, 5)
        # the C entry: a status and mdl_last_error
        L = _lib.lib()
        out = torch.empty_like(want)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for args, word in (((0, 4, None, 0, out.data_ptr()), "radius"), ((0, 4, None, 16, out.data_ptr()), "radius"),
                           ((1, 4, None, 2, out.data_ptr()), "range"), ((0, 4, ok.data_ptr(), 2, None), "null output")):
            assert L.mdl_build_obs_alt_ego(env._h, *args, s) != 0, args
            assert word in L.mdl_last_error().decode(), (args, L.mdl_last_error())
        assert L.mdl_build_obs_alt_ego(env._h, 2, 0, None, 2, None, s) == 0   # n == 0 launches nothing
        assert L.mdl_build_obs_alt_ego(env._h, 0, 4, ok.data_ptr(), 2, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(env.build_obs_alt_ego(2, rows=ok), want)
    finally:
        env.close()


# ---------------------------------------------------------------- 4. capture
def test_captured_masked_call_follows_the_mask():
    case = X.BY_ID["m1_a5_stale"]
    R, E = 2, case.E
    env = make_env(case)
    try:
        env.reset()
        tr = X.trace(case)
        for k, ints, dn, full in tr[:4]:
            if ints is not None:
                env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
        assert tr[3][0] == 2 and tr[3][3] is not None   # step 2 is a build point
        want = windows(tr[3][3], R)
        mask = dev_mask(M.mask_patterns(E)["even"])
        out = torch.empty((E,) + want.shape[1:], dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            env.build_obs_alt_ego(R, rows=mask, out=out)   # warm-up
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                env.build_obs_alt_ego(R, rows=mask, out=out)
        torch.cuda.synchronize()
        for name in ("even", "odd", "bytes", "none"):
            m = M.mask_patterns(E)[name]
            mask.copy_(torch.from_numpy(m))
            out.view(torch.int32).fill_(int(SENT))
            g.replay()
            torch.cuda.synchronize()
            got = raw(out)
            for e in range(E):
                if m[e]:
                    assert got[e].tobytes() == want[e].tobytes(), f"replay under mask {name}: env {e}"
                else:
                    assert (got[e] == SENT).all(), f"replay under mask {name}: env {e} was written"
    finally:
        env.close()
