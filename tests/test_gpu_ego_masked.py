"""Masked actor-map windows (BatchedEnv.build_obs_ego_masked, k_masked_ego_maps) and the episode loops on
them.  The kernel under row masks against ego_ref.ego_from_full of the ORACLE's actor map, bit for bit, the
rows of unmarked envs against a sentinel byte for byte; past one workgroup and one XCD round; the refusals;
step_episode + masked windows over episodes that end at different steps (ego_masked_ref.EPISODE, whose input
conditions test_ego_masked_cpu.py pins on the oracle); QmixCollector(ego_radius=) against a full-map twin;
EpisodeReplay on a window-form template; Evaluator(ego_radius=)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ego_masked_ref as M  # noqa: E402
import ego_ref as G  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
ONE = {torch.float32: 0x3F800000, torch.float16: 0x3C00, torch.bfloat16: 0x3F80}
INT_VIEW = {4: torch.int32, 2: torch.int16}
NP_VIEW = {4: np.uint32, 2: np.uint16}
GUARD = 8


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


def sentinel_(t):
    """Fill t with the sentinel bit pattern of its element size."""
    t.view(INT_VIEW[t.element_size()]).fill_(M.SENTINEL_BITS[t.element_size()])
    return t


def sentinel(shape, dtype):
    return sentinel_(torch.empty(shape, dtype=dtype, device="cuda"))


def raw(t):
    """The elements' bit patterns on the host."""
    return t.detach().contiguous().view(INT_VIEW[t.element_size()]).cpu().numpy().view(NP_VIEW[t.element_size()])


def want_bits(want, dtype):
    """The oracle's float32 windows (0 and 1 only) as the bit patterns of `dtype`."""
    assert set(np.unique(want)) <= {0.0, 1.0}
    return want.astype(NP_VIEW[torch.empty(0, dtype=dtype).element_size()]) * ONE[dtype]


def windows(full, R):
    return np.stack([G.ego_from_full(f, R) for f in full])   # [E, A, 6, K, K]


def check_rows(got, want, sel, what):
    """got, want [n, ...] bit patterns, sel bool [n]: marked rows are the oracle's, the others the sentinel."""
    sent = got.dtype.type(M.SENTINEL_BITS[got.dtype.itemsize])
    for i in range(len(sel)):
        if sel[i]:
            if got[i].tobytes() != want[i].tobytes():
                bad = np.argwhere(got[i] != want[i])
                raise AssertionError(f"{what}: row {i}: {len(bad)} elements differ from the oracle, first at "
                                     f"(robot, channel, row, col) {tuple(bad[0])}")
        else:
            assert (got[i] == sent).all(), f"{what}: row {i} is unmarked and was written"


def dev_mask(m):
    return torch.from_numpy(np.ascontiguousarray(m, np.uint8)).cuda()


def masked_builds(env, R, full, what, masks, b0=0, n=None):
    """Every mask x dtype over envs [b0, b0 + n) against the oracle; with a sub-range the rows lie in one
    larger allocation between sentinel guards, row 0 on a 4-byte but not a 16-byte line."""
    E = env.E
    n = E - b0 if n is None else n
    want = windows(full, R)[b0:b0 + n]
    sub = (b0, n) != (0, E)
    for dt in DTYPES:
        wb = want_bits(want, dt)
        row = wb[0].size
        es = torch.empty(0, dtype=dt).element_size()
        lead = 4 // es if sub else 0
        per = GUARD + lead + n * row + GUARD
        per += (-per * es % 16) // es   # every mask's slice starts on a 16-byte line (es divides 16)
        buf = sentinel((len(masks), per), dt)
        assert buf.data_ptr() % 16 == 0 and per * es % 16 == 0
        for i, (name, m) in enumerate(masks.items()):
            out = buf[i, GUARD + lead:GUARD + lead + n * row].view(wb.shape)
            assert out.data_ptr() % 16 == (lead * es) % 16 and out.data_ptr() % 4 == 0
            got = env.build_obs_ego_masked(R, dev_mask(m), env_begin=b0, n=n, out=out, dtype=dt)
            assert got.data_ptr() == out.data_ptr()
        plain = raw(env.build_obs_ego(R, env_begin=b0, n=n, dtype=dt))
        host = raw(buf)
        sent = host.dtype.type(M.SENTINEL_BITS[es])
        for i, (name, m) in enumerate(masks.items()):
            w = f"{what} mask {name} envs [{b0}, {b0 + n}) as {dt}"
            got = host[i, GUARD + lead:GUARD + lead + n * row].reshape(wb.shape)
            check_rows(got, wb, m[b0:b0 + n] != 0, w)
            assert (host[i, :GUARD + lead] == sent).all() and (host[i, GUARD + lead + n * row:] == sent).all(), \
                f"{w}: a guard element was overwritten"
            if (m[b0:b0 + n] != 0).all():
                assert got.tobytes() == plain.tobytes(), f"{w}: differs from the unmasked build"


# ---------------------------------------------------------------- 1. the kernel under masks
@pytest.mark.parametrize("cid", M.KERNEL_CASES)
def test_masked_windows_vs_oracle(cid):
    case = G.BY_ID[cid]
    env = make_env(case)
    E = case.E
    masks = M.mask_patterns(E)
    pts = G.build_points(case)
    sub_at = next(k for k in pts if k > case.T)   # past the first auto-reset
    try:
        env.reset()
        for k, ints, dn, full in G.trace(case):
            if ints is not None:
                env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
            if full is None:
                continue
            for R in case.radii:
                masked_builds(env, R, full, f"{cid} step {k} R={R}", masks)
                if k == sub_at:   # the mask stays indexed by env id; mixed_stale crosses both map boundaries
                    masked_builds(env, R, full, f"{cid} step {k} R={R}", masks, b0=1, n=E - 2)
                    if E > 4:
                        masked_builds(env, R, full, f"{cid} step {k} R={R}", masks, b0=3, n=E - 4)
        # a fresh tensor under a mask starts as zeros
        m = masks["even"]
        z = env.build_obs_ego_masked(case.radii[0], dev_mask(m))
        assert not raw(z)[m == 0].any() and raw(z)[m != 0].any()
    finally:
        env.close()


# ---------------------------------------------------------------- 2. many workgroups
def test_masks_past_one_workgroup_and_xcd_round():
    case = M.BIG
    env = make_env(case)
    masks = M.big_masks()
    try:
        env.reset()
        n = 0
        for k, ints, dn, full in G.trace(case):
            if ints is not None:
                env.step(torch.from_numpy(ints).cuda(), auto_reset=True)
            if full is None:
                continue
            masked_builds(env, 2, full, f"{case.id} step {k}", masks)
            n += 1
        masked_builds(env, 2, full, f"{case.id} last", masks, b0=5, n=59)
        assert n >= 3
    finally:
        env.close()


# ---------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_engine_usable():
    import marl_gpu
    from marl_gpu import _lib
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 4, 3, 8, 10, seed=1)
    try:
        env.reset()
        ok = torch.ones(4, dtype=torch.uint8, device="cuda")
        want = env.build_obs_ego(2)
        with pytest.raises(TypeError, match="rows"):
            env.build_obs_ego_masked(2, ok.to(torch.int32))
        with pytest.raises(TypeError, match="rows"):
            env.build_obs_ego_masked(2, ok.bool())
        with pytest.raises(TypeError, match="rows"):
            env.build_obs_ego_masked(2, None)
        with pytest.raises(ValueError, match="rows"):
            env.build_obs_ego_masked(2, ok[:3])
        with pytest.raises(ValueError, match="rows"):
            env.build_obs_ego_masked(2, ok.cpu())
        with pytest.raises(ValueError, match="rows"):
            env.build_obs_ego_masked(2, torch.ones(8, dtype=torch.uint8, device="cuda")[::2])
        for R in (0, 16):
            with pytest.raises(ValueError, match="radius"):
                env.build_obs_ego_masked(R, ok)
        with pytest.raises(IndexError):
            env.build_obs_ego_masked(2, ok, env_begin=2, n=3)
        # the C entry: a status and mdl_last_error
        L = _lib.lib()
        out = env.ego_buffers(2)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.mdl_build_obs_ego_masked(env._h, 0, 4, None, 2, 0, out.data_ptr(), s) != 0
        assert "rows" in L.mdl_last_error().decode()
        for args, word in (((0, 4, ok.data_ptr(), 0, 0), "radius"), ((0, 4, ok.data_ptr(), 16, 0), "radius"),
                           ((0, 4, ok.data_ptr(), 2, 3), "dtype"), ((1, 4, ok.data_ptr(), 2, 0), "range")):
            assert L.mdl_build_obs_ego_masked(env._h, *args, out.data_ptr(), s) != 0, args
            assert word in L.mdl_last_error().decode(), (args, L.mdl_last_error())
        assert L.mdl_build_obs_ego_masked(env._h, 0, 4, ok.data_ptr(), 2, 0, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(env.build_obs_ego_masked(2, ok), want)
    finally:
        env.close()


@pytest.mark.skipif(torch.cuda.is_available() and torch.cuda.device_count() < 2, reason="needs a second device")
def test_rows_on_another_device_are_refused():
    import marl_gpu
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 4, 3, 8, 10, seed=1)
    try:
        env.reset()
        with pytest.raises(ValueError, match="rows"):
            env.build_obs_ego_masked(2, torch.ones(4, dtype=torch.uint8, device="cuda:1"))
        assert tuple(env.build_obs_ego_masked(2, torch.ones(4, dtype=torch.uint8, device="cuda")).shape) == (4, 3, 6, 5, 5)
    finally:
        env.close()


# ---------------------------------------------------------------- 4. step_episode + masked windows
def episode_env(ep=M.EPISODE):
    import marl_gpu
    return marl_gpu.BatchedEnv(grid(ep.map), ep.E, ep.A, ep.P, ep.T, seed=ep.seed, tracker="fresh", shaping="qmix")


def test_step_episode_with_masked_windows_over_staggered_episodes():
    ep = M.EPISODE
    tr = M.episode_trace(ep)
    R, E = ep.R, ep.E
    K = 2 * R + 1
    env = episode_env()
    d = M.EpisodeDriver(ep)
    try:
        env.reset()
        env.greedy_init()
        active = torch.ones(E, dtype=torch.uint8, device="cuda")
        filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
        ego = {dt: sentinel((E, ep.A, 6, K, K), dt) for dt in DTYPES}
        for dt in DTYPES:
            env.build_obs_ego(R, out=ego[dt], dtype=dt)
            check_rows(raw(ego[dt]), want_bits(windows(tr["full0"], R), dt), np.ones(E, bool), f"after reset as {dt}")
        terminal = kept = 0
        for k in range(ep.T):
            codes = env.greedy_actions_masked(active)
            ints = M.codes_to_ints(codes.cpu().numpy())
            run = tr["filled"][k]
            assert np.array_equal(ints[run], tr["ints"][k][run]), f"step {k}: the device's greedy actions"
            env.step_episode(codes, active, action_format="codes", filled=filled, which=())
            prev = {dt: raw(ego[dt]).copy() for dt in DTYPES}
            for dt in DTYPES:
                env.build_obs_ego_masked(R, filled, out=ego[dt], dtype=dt)
            f = filled.cpu().numpy().astype(bool)
            a = active.cpu().numpy().astype(bool)
            assert np.array_equal(f, run), f"step {k}: filled"
            dn = d.step(ints, f)
            assert np.array_equal(a, f & ~dn), f"step {k}: active after the step"
            terminal += int((f & ~a).sum())   # written under `filled`, lost under `active`
            for dt in DTYPES:
                got = raw(ego[dt])
                for e in range(E):
                    if f[e]:
                        want = want_bits(G.ego_from_full(d.full(e), R), dt)
                        assert got[e].tobytes() == want.tobytes(), \
                            f"step {k} env {e} as {dt}{' (terminal state)' if dn[e] else ''}: differs from the oracle"
                    else:
                        kept += 1
                        assert got[e].tobytes() == prev[dt][e].tobytes(), f"step {k} env {e} as {dt}: an idle row changed"
        assert terminal == E and kept > 0 and not active.cpu().numpy().any()
    finally:
        env.close()


# ---------------------------------------------------------------- 5. QmixCollector
class GreedyQ:
    """A QMIX agent whose q is a one-hot of the device's greedy action (as a trainer int) plus a small
    fixed linear map of vo: a function of vo, h and the engine state alone, never of so, so a window-form
    collector and its full-map twin choose the same actions -- and the deliveries end episodes early."""
    HD = 8

    def __init__(self, env, gen_seed=11):
        self.env = env
        self.col = None
        gen = torch.Generator(device="cuda").manual_seed(gen_seed)
        self.wq = torch.randn(env.actor_vec_dim, 15, device="cuda", generator=gen) * 1e-3
        self.wh = torch.randn(env.actor_vec_dim, self.HD, device="cuda", generator=gen) * 0.1
        self.lut = torch.from_numpy(M.INT_OF_CODE.astype(np.int64)).cuda()
        self.seen = []

    def init_hidden(self):   # called once per collect, right after the reset
        self.env.greedy_init()
        return torch.zeros(1, self.HD, device="cuda")

    def __call__(self, so, vo, h):
        self.seen.append((tuple(so.shape), so.dtype))
        codes = self.env.greedy_actions_masked(self.col.active)
        ints = self.lut[codes.view(-1).long()]
        q = (vo @ self.wq).clamp_(-1.0, 1.0)
        q.scatter_add_(1, ints.unsqueeze(1), torch.full((q.shape[0], 1), 10.0, device="cuda"))
        return q, torch.tanh(0.5 * h + vo @ self.wh)


def make_collector(**kw):
    from marl_gpu.qmix_rollout import QmixCollector
    env = episode_env()
    ag = GreedyQ(env)
    col = QmixCollector(env, M.EPISODE.T, seed=3, **kw)
    ag.col = col
    return env, ag, col


SAME = ("vo", "gs", "gv", "u", "r", "r64", "r_shaped", "terminated", "filled", "episode_return", "episode_length")


def check_against_twin(full, ego, R, dt, what):
    for k in SAME:
        assert torch.equal(full[k], ego[k]), f"{what}: {k}"
    assert torch.equal(full["hidden"], ego["hidden"]), f"{what}: hidden"
    L, E = ego["filled"].shape
    f = ego["filled"].cpu().numpy().astype(bool)
    got = raw(ego["so"])
    maps = full["so"].cpu().numpy()
    assert ego["so"].dtype == dt and got.shape[:3] == maps.shape[:3]
    for t in range(L + 1):   # the twin's rows past an episode's end hold no observation: only written rows are cropped
        sel = np.ones(E, bool) if t == 0 else f[t - 1]
        want = np.zeros_like(got[t])
        want[sel] = want_bits(G.ego_from_full(maps[t][sel], R), dt)
        check_rows(got[t], want, sel, f"{what}: slot {t}")
    return f


@pytest.mark.parametrize("dt,avail", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)],
                         ids=["float32", "bfloat16", "float32-avail"])
def test_qmix_collector_with_windows_against_a_full_map_twin(dt, avail):
    ep = M.EPISODE
    R, K = ep.R, 2 * ep.R + 1
    made = [make_collector(avail=avail), make_collector(avail=avail, ego_radius=R, ego_dtype=dt)]
    try:
        (_, ag_f, full), (_, ag_e, ego) = made
        assert tuple(ego.so.shape) == (ep.T + 1, ep.E, ep.A, 6, K, K) and ego.so.dtype == dt
        assert tuple(full.so.shape) == (ep.T + 1, ep.E, ep.A, 6, 10, 10)
        for call in range(2):   # the second collect plays the next layouts of the same streams
            sentinel_(ego.so)
            bf = full.collect(ag_f, 0.0)
            be = ego.collect(ag_e, 0.0)
            torch.cuda.synchronize()
            f = check_against_twin(bf, be, R, dt, f"collect {call}")
            if call == 0 and not avail:   # the episodes are ego_masked_ref's: they end at different steps
                assert np.array_equal(f, M.episode_trace(ep)["filled"])
                assert np.array_equal(be["u"].cpu().numpy()[f], M.episode_trace(ep)["ints"][f])
            if avail:
                assert torch.equal(bf["avail"], be["avail"])
        assert ag_e.seen[0] == ((ep.E * ep.A, 6, K, K), dt) and ag_f.seen[0] == ((ep.E * ep.A, 6, 10, 10), torch.float32)
    finally:
        for env, _, _ in made:
            env.close()


def test_qmix_collector_with_windows_graph_equals_eager():
    ep = M.EPISODE
    made = [make_collector(ego_radius=ep.R), make_collector(ego_radius=ep.R)]
    try:
        (_, ag_a, eager), (_, ag_b, graphed) = made
        for call in range(3):   # call 0 of `graphed` runs eagerly and captures, calls 1 and 2 replay
            sentinel_(eager.so)
            sentinel_(graphed.so)
            a = eager.collect(ag_a, 0.0)
            b = graphed.collect(ag_b, 0.0, graph=True)
            torch.cuda.synchronize()
            for k in SAME + ("hidden",):
                assert torch.equal(a[k], b[k]), f"collect {call}: {k}"
            assert raw(a["so"]).tobytes() == raw(b["so"]).tobytes(), f"collect {call}: so"
            if call == 0:   # ego_masked_ref's episodes: some end early, so rows stay unwritten
                assert not a["filled"].all() and (raw(b["so"]) == M.SENTINEL_BITS[4]).any()
        assert graphed.captured_graphs() == {None: ep.T}
    finally:
        for env, _, _ in made:
            env.close()


# ---------------------------------------------------------------- 6. EpisodeReplay
def test_episode_replay_on_a_window_template():
    from marl_gpu.replay import EpisodeReplay
    ep = M.EPISODE
    R, K = ep.R, 2 * ep.R + 1
    env, ag, col = make_collector(ego_radius=R, ego_dtype=torch.bfloat16)
    try:
        rep = EpisodeReplay(2 * ep.E, col)
        assert tuple(rep.buf["so"].shape) == (ep.T + 1, 2 * ep.E, ep.A, 6, K, K) and rep.buf["so"].dtype == torch.bfloat16
        batch = col.collect(ag, 0.0)
        rep.add(batch)
        B = 5
        s = rep.sample(B, generator=torch.Generator().manual_seed(1))
        for k in ("so", "so_next"):
            assert tuple(s[k].shape) == (B, ep.T, ep.A, 6, K, K) and s[k].dtype == torch.bfloat16, k
        u = batch["u"].transpose(0, 1).long().unsqueeze(-1)   # [E, L, A, 1]
        r = batch["r"].transpose(0, 1).unsqueeze(-1)
        so = batch["so"].transpose(0, 1)
        for b in range(B):
            hit = [e for e in range(ep.E) if torch.equal(u[e], s["u"][b]) and torch.equal(r[e], s["r"][b])]
            assert hit, f"sample {b} is none of the collected episodes"
            assert any(raw(so[e][:-1]).tobytes() == raw(s["so"][b]).tobytes()
                       and raw(so[e][1:]).tobytes() == raw(s["so_next"][b]).tobytes() for e in hit), f"sample {b}: so"
    finally:
        env.close()


# ---------------------------------------------------------------- 7. Evaluator
def test_evaluator_with_windows():
    import marl_gpu
    from marl_gpu.evaluate import Evaluator
    E, A, P, T, R = 8, 3, 3, 12, 2
    K = 2 * R + 1
    g = grid("map1.txt")

    def make():
        return marl_gpu.BatchedEnv(g, E, A, P, T, seeds=[500 + i for i in range(E)], tracker="fresh")

    envs = [make() for _ in range(5)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    w = torch.randn(envs[0].actor_vec_dim, 15, device="cuda", generator=gen)
    seen = []

    def policy(om, ov):   # reads the vector alone
        return ov @ w

    def recorder(om, ov):
        if not seen:
            seen.append(om.clone())
        return ov @ w

    try:
        plain, ego, graphed = Evaluator(envs[0], seed=2), Evaluator(envs[1], seed=2, ego_radius=R), \
            Evaluator(envs[2], seed=2, ego_radius=R)
        for call, det in enumerate((True, True, False, False)):
            a = {k: v.clone() for k, v in plain.run(policy, deterministic=det).items()}
            b = {k: v.clone() for k, v in ego.run(policy, deterministic=det).items()}
            c = {k: v.clone() for k, v in graphed.run(policy, deterministic=det, graph=True, graph_steps=5).items()}
            torch.cuda.synchronize()
            for k in ("rewards", "delivered", "steps", "finished"):
                assert torch.equal(a[k], b[k]), f"run {call}: {k}, windows against the full map"
                assert torch.equal(a[k], c[k]), f"run {call}: {k}, graphed windows"
        # the policy receives the windows of the reset state, in the evaluator's dtype
        half = Evaluator(envs[3], seed=2, ego_radius=R, ego_dtype=torch.bfloat16)
        half.run(recorder, max_steps=2)
        envs[4].reset()
        full = envs[4].build_obs()["actor_map"].cpu().numpy()
        assert seen[0].dtype == torch.bfloat16 and tuple(seen[0].shape) == (E * A, 6, K, K)
        want = want_bits(G.ego_from_full(full, R), torch.bfloat16).reshape(E * A, 6, K, K)
        assert raw(seen[0]).tobytes() == want.tobytes()
        # run_eval passes the option through: the same summary with and without windows
        from marl_gpu.evaluate import run_eval
        cfg = dict(map=g, max_time_steps=T, n_agents=A, n_packages=P, seed=500)
        s0 = run_eval("mappo", cfg, E, policy=policy, deterministic=True)
        shapes = []

        def shape_policy(om, ov):
            shapes.append((tuple(om.shape), om.dtype))
            return ov @ w

        s1 = run_eval("mappo", cfg, E, policy=shape_policy, deterministic=True, ego_radius=R, ego_dtype=torch.float16)
        assert s0["rewards"] == s1["rewards"] and s0["delivered"] == s1["delivered"]
        assert shapes[0] == ((E * A, 6, K, K), torch.float16)
        # the greedy kind ignores the option
        r0 = {k: v.clone() for k, v in Evaluator(envs[3], ego_radius=R).run("greedy").items()}
        r1 = Evaluator(envs[4]).run("greedy")
        for k in r0:
            assert torch.equal(r0[k], r1[k]), k
    finally:
        for e in envs:
            e.close()
