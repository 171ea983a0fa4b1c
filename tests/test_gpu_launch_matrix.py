"""Every reset, cycle-begin and alt-builder kernel (tests/launch_matrix.py: 21 symbols) against the CPU
oracle, bit for bit: the seeding, explicit resets of id lists, device id tensors and all envs on fresh
and stale trackers (through reset and mail_reset), the tracker clear mid-episode, the map-QMIX cycle's
lazy reset at every package-chunk class, the IDQ / qmix builders on trackers that hold survivors of
earlier episodes, one engine that mixes two maps of a shape, and storms of resets that reach the edges
of the draw stream (refills, rejections, retries, ranges of one value).

Each case first runs the oracle alone (tests/launch_ref.py: every call's expected results) and asserts
on that trace that the inputs reach what the case is there for, before the engine runs against it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import launch_ref as R  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402
from launch_matrix import CASES, EXCLUDED, case_id  # noqa: E402
from step_matrix import codes_of  # noqa: E402
from test_gpu_step_matrix import check_out, check_state, same  # noqa: E402

NAN_BITS = np.uint32(0x7FC00BAD)   # a quiet NaN no builder writes: the "row not written" sentinel


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_filled(shape):
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def unwritten(x, what):
    assert (np.asarray(x).view(np.uint32) == NAN_BITS).all(), f"{what}: rows of other envs were written"


def acts(tracker, ints):
    """(format, device tensor): trainer ints on the stale tracker, the same actions as code bytes on the fresh."""
    fmt = "int" if tracker == "mappo" else "codes"
    return fmt, dev(ints if fmt == "int" else codes_of(ints))


def kinds(kind):
    cs = [c for c in CASES if c.kind in kind and c.symbol not in EXCLUDED]
    return dict(argvalues=cs, ids=[case_id(c) for c in cs])


def make_engine(mg, case, grids=None, env_map=None):
    return mg.BatchedEnv(grid(case.map) if grids is None else grids, case.E, case.A, case.P, case.T, seed=case.seed,
                         tracker=case.tracker, shaping="mappo", env_map=env_map)


# ------------------------------------------------------------------ k_seed, k_reset, k_tracker_clear
def check_mailbox(env, mb, ids, s, what):
    """The mailbox rows of the call's envs against read_state, as the step matrix's mailbox run checks them."""
    n = len(ids)
    same(mb["robots"][:n].copy(), s["robots"][ids], f"{what}: mailbox robot rows")
    same(mb["pkgs"][:n].copy(), s["pkgs"][ids], f"{what}: mailbox package rows")
    same(mb["t"][:n].copy(), s["t"][ids], f"{what}: mailbox t")
    same(mb["total_reward"][:n].copy(), s["total_reward"][ids], f"{what}: mailbox total_reward")


def run_reset(case, env, trace):
    mb = env.mailbox() if case.mail else None
    for k, c in enumerate(trace):
        what = f"call {k} ({c['op']})"
        if c["op"] == "seed":
            pass                                           # the constructor ran k_seed
        elif c["op"] == "step":
            fmt, a = acts(case.tracker, c["ints"])
            r, sh, dn = env.step(a, auto_reset=False, action_format=fmt)
            check_out(r, sh, dn, c, what)
        elif c["op"] == "clear":
            env.clear_tracker(c["ids"])
        elif case.mail and c.get("explicit"):
            ids = c["ids"]
            if c["given"] is not None:
                mb["ids"][:len(ids)] = ids
            env.mail_reset(len(ids), c["given"] is not None)
            check_mailbox(env, mb, ids, check_state(env, c["state"], what), what)
            continue
        elif c["given"] is not None and c.get("explicit") == 2:
            env.reset(torch.tensor(c["given"], dtype=torch.int32, device="cuda"))
        else:
            env.reset(c["given"])
        check_state(env, c["state"], what)


@pytest.mark.parametrize("case", **kinds(("seed", "reset")))
def test_reset_kernels_vs_oracle(case):
    import marl_gpu
    trace = R.reset_trace(case)
    R.check_reset_inputs(case, trace)
    env = make_engine(marl_gpu, case)
    try:
        run_reset(case, env, trace)
    finally:
        env.close()


# ------------------------------------------------------------------ k_cycle_begin
def make_cycle_engine(mg, case, grids=None, env_map=None):
    """The trainer's constructor: the tracker is empty when the first reset fills it."""
    env = make_engine(mg, case, grids, env_map)
    if case.tracker != "fresh":
        env.clear_tracker()
    env.reset()
    return env


def run_cycle(case, a, b, trace, H, W):
    """Engine a runs cycle_begin, its twin b clear_tracker + reset; both step alike."""
    E, A = case.E, case.A
    for k, c in enumerate(trace):
        what = f"call {k} ({c['op']})"
        if c["op"] == "step":
            fmt, x = acts(case.tracker, c["ints"])
            r, _, dn = a.step(x, auto_reset=False, action_format=fmt)
            same(host(r), c["r"], f"{what}: r_env")
            same(host(dn).astype(bool), c["done"], f"{what}: done")
            b.step(x, auto_reset=False, action_format=fmt)
            check_state(a, c["state"], what)
            continue
        done = dev(c["mask"])
        out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E, 7, H, W)))
        completed = torch.full((E,), 0xA5, dtype=torch.uint8, device="cuda")
        c_ret = torch.full((E,), -7.5, dtype=torch.float64, device="cuda")
        c_steps = torch.full((E,), -3, dtype=torch.int32, device="cuda")
        a.cycle_begin(done, out=out, completed=completed, completed_return=c_ret, completed_steps=c_steps)
        check_state(a, c["state"], what)
        same(host(completed), c["mask"], f"{what}: completed")
        same(host(c_ret), c["ret"], f"{what}: completed_return")
        same(host(c_steps), c["steps"], f"{what}: completed_steps")
        assert not host(done).any(), f"{what}: the mask is consumed"
        idq, qst = host(out["idq_obs"]), host(out["qmix_state"])
        off = [e for e in range(E) if e not in c["ids"]]
        for e in c["ids"]:
            same(idq[e], c["obs"][e][0], f"{what}: idq_obs of env {e}")
            same(qst[e], c["obs"][e][1], f"{what}: qmix_state of env {e}")
        unwritten(idq[off], f"{what}: idq_obs")
        unwritten(qst[off], f"{what}: qmix_state")
        b.clear_tracker(c["ids"])
        b.reset(c["ids"])
        assert a.save_state().tobytes() == b.save_state().tobytes(), f"{what}: engine state != clear_tracker + reset"


@pytest.mark.parametrize("case", **kinds(("cycle",)))
def test_cycle_begin_vs_oracle(case):
    import marl_gpu
    trace = R.cycle_trace(case)
    R.check_cycle_inputs(case, trace)
    H, W = grid(case.map).shape
    a, b = make_cycle_engine(marl_gpu, case), make_cycle_engine(marl_gpu, case)
    try:
        run_cycle(case, a, b, trace, H, W)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ k_alt_obs, k_alt_transition
@pytest.mark.parametrize("case", **kinds(("alt",)))
def test_alt_builders_vs_oracle(case):
    import marl_gpu
    H, W = grid(case.map).shape
    other = (7, H + 3, W - 2)
    trace = R.alt_trace(case, other)
    R.check_alt_inputs(case, trace)
    E, A = case.E, case.A
    env = make_engine(marl_gpu, case)
    try:
        env.reset()
        pre = env.alt_pre_buffer()
        for k, c in enumerate(trace):
            what = f"call {k} ({c['op']})"
            out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E, 7, H, W)))
            if c["op"] == "begin":
                r, o = env.alt_transition(None, pre, out=out, which=("idq_obs", "qmix_state"))
                assert r is None
            else:
                x = dev(c["ints"])
                _, _, dn = env.step(x, auto_reset=True)
                same(host(dn).astype(bool), c["done"], f"{what}: done")
                r, o = env.alt_transition(x, pre, ops_are_ints=True, out=out, which=("idq_obs", "qmix_state"))
                same(host(r), c["r_idq"], f"{what}: IDQ reward")
            check_state(env, c["state"], what)
            same(host(o["idq_obs"]), c["obs"]["idq"], f"{what}: alt_transition idq_obs")
            same(host(o["qmix_state"]), c["obs"]["qst"], f"{what}: alt_transition qmix_state")
            alt = env.build_obs_alt()
            same(host(alt["idq_obs"]), c["obs"]["idq"], f"{what}: build_obs_alt idq_obs")
            same(host(alt["qmix_state"]), c["obs"]["qst"], f"{what}: build_obs_alt qmix_state")
            alt = env.build_obs_alt(state_shape=other, which=("qmix_state",))
            same(host(alt["qmix_state"]), c["obs"]["other"], f"{what}: build_obs_alt qmix_state {other}")
    finally:
        env.close()


# ------------------------------------------------------------------ two maps of one shape in one engine
MULTI_ENV_MAP = [0, 1, 1, 0, 1, 0]


def multi_grids():
    """map1.txt and a flipped copy.  map1.txt is a walled square, which every flip maps onto itself, so
    the copy first gets three interior walls: another free-cell list, and another free-cell count."""
    g = grid("map1.txt")
    f = g.copy()
    f[1, 1] = f[2, 5] = f[7, 3] = 1
    f = np.ascontiguousarray(f[::-1])
    assert f.shape == g.shape == (10, 10) and int((f == 0).sum()) == int((g == 0).sum()) - 3
    assert not np.array_equal(f, f[::-1]) and not np.array_equal(f, g)
    return [g, f]


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
def test_same_shape_maps_reset_and_cycle_vs_oracle(tracker):
    """p.env_map, md.free_off and md.nfree in k_seed, k_reset, k_tracker_clear and k_cycle_begin: one
    engine over map1.txt and a flipped copy, a non-constant env_map, one oracle per env."""
    import marl_gpu
    from launch_matrix import Case
    maps = multi_grids()
    per_env = [maps[m] for m in MULTI_ENV_MAP]
    assert len(set(MULTI_ENV_MAP)) == 2 and MULTI_ENV_MAP != sorted(MULTI_ENV_MAP)
    case = Case("multi-map", "reset", "map1.txt", 5, 65, tracker, E=len(MULTI_ENV_MAP), seed=31)
    trace = R.reset_trace(case, per_env)
    R.check_reset_inputs(case, trace)
    seeded = trace[0]["state"]
    assert any(not np.array_equal(seeded["robots"][e], R.Envs(maps[1 - m], 1, case.A, case.P, case.T, case.seed + e,
                                                              tracker, constructed=True).state()["robots"][0])
               for e, m in enumerate(MULTI_ENV_MAP)), "the two maps must draw different layouts"
    env = make_engine(marl_gpu, case, maps, MULTI_ENV_MAP)
    try:
        run_reset(case, env, trace)
    finally:
        env.close()
    ctrace = R.cycle_trace(case, per_env)
    R.check_cycle_inputs(case, ctrace)
    a, b = (make_cycle_engine(marl_gpu, case, maps, MULTI_ENV_MAP) for _ in range(2))
    try:
        run_cycle(case, a, b, ctrace, 10, 10)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ the reset storm
@pytest.mark.parametrize("name", sorted(R.STORM))
def test_reset_storm(name):
    import marl_gpu
    trace = R.storm_trace(name)
    R.check_storm_inputs(name, trace)
    mk, A, P, T, E, tracker, _ = R.STORM[name]
    env = marl_gpu.BatchedEnv(mk(), E, A, P, T, seed=R.STORM_SEED, tracker=tracker)
    try:
        env.reset()
        for k, c in enumerate(trace):
            env.reset()
            check_state(env, c["state"], f"reset {k}")
    finally:
        env.close()
