"""Device-resident IDQ collection: the masked transition launch (``BatchedEnv.alt_transition``:
reward_shaping from the pre-record, next observations) against the CPU oracle along masked
episodes, on the fast and the general emit path; the compacting replay append
(``TransitionReplay.add``) against the reference's sequential ``ReplayBuffer.add`` restated in
numpy; and ``IdqCollector`` against a hand-written loop and against its own hipGraph replay.
Everything is compared bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402

NAN_BITS = np.uint32(0x7FC00BAD)   # a quiet NaN no builder writes: the "row not written" sentinel
TRAINER_MOVE = [O.MOVE_CODES[c] for c in O.TRAINER_MOVES]   # LabelEncoder order D, L, R, S, U


def bits(t):
    """Bit pattern of a float tensor / array as a numpy integer array (-0.0 != 0.0, NaNs compare)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def nan_filled(shape):
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(np.float32)).cuda()


def decode(ints):
    """Trainer ints -> (move codes, op codes), IDQ/trainer.py:273-279 (== MAPPO/trainer.py:198-205)."""
    ints = np.asarray(ints).astype(np.int64)
    op = ints // 5
    return np.array([TRAINER_MOVE[m] for m in ints % 5], np.uint8), np.where(op >= 3, 0, op).astype(np.uint8)


class OracleEpisodes:
    """E oracle envs with per-episode trackers, stepped under a caller's mask without reset
    (what step_episode + alt_transition do), yielding what the IDQ trainer computes per step."""

    def __init__(self, g, E, A, P, T, seed):
        self.g, self.E, self.A = g, E, A
        self.ob = O.OracleBatch(E, g, A, P, T, seed_base=seed, clear_on_reset=True)

    def view(self, e):
        """(t, robots 1-indexed, tracker rows) of env e now."""
        env = self.ob.env(e)
        return env.state()["t"], env.robots1(), self.ob.tracker(e).rows()

    def obs(self, e, state_shape):
        t, r1, rows = self.view(e)
        idq = np.stack([O.idq_convert_state(self.g, t, r1, rows, a) for a in range(self.A)])
        return idq, O.qmix_global_tensor(self.g, t, r1, rows, state_shape)

    def step(self, e, ints, ops_are_ints):
        """One transition of env e: (r_idq f64 [A], done, tags) with the pre-step tracker rows."""
        pt, pr1, rows = self.view(e)
        mv, op = decode(ints)
        env = self.ob.env(e)
        _, _, done = env.step(mv, op)
        self.ob.tracker(e).update_from_env(env)
        ct, cr1, _ = self.view(e)
        r = O.idq_reward_shaping(pt, pr1, ct, cr1, op, ops_are_ints, rows, self.A)
        pcy, ccy = pr1[:, 2], cr1[:, 2]
        tags = dict(pickup=int(((op == 1) & (pcy == 0) & (ccy != 0)).sum()), delivery=int((r >= 4.0).sum()),
                    wasted=int(((op == 1) & (pcy != 0)).sum()))
        return r, done, tags


def masked_run(cfg, seed, n_steps, ops_are_ints):
    """The oracle side of test 1, usable without a GPU: yields per step (ints, mask before the step,
    {e: (r, idq, qst)} for the stepped envs, mask after it, tags)."""
    mapname, A, P, T, E = cfg
    g = grid(mapname)
    H, W = g.shape
    orc = OracleEpisodes(g, E, A, P, T, seed)
    rs = np.random.RandomState(seed)
    mask = np.ones(E, bool)
    mask[::3] = False                     # a third of the envs never runs
    yield orc, mask.copy()
    for k in range(n_steps):
        if k == 7:
            mask[[1, 4]] = False          # two episodes cut by the caller
        ints = rs.randint(0, 15, size=(E, A)).astype(np.uint8)
        before = mask.copy()
        want, tags = {}, dict(pickup=0, delivery=0, wasted=0)
        for e in np.nonzero(before)[0]:
            r, done, tg = orc.step(e, ints[e], ops_are_ints)
            want[e] = (r,) + orc.obs(e, (7, H, W))
            mask[e] = not done
            for kk in tags:
                tags[kk] += tg[kk]
        yield ints, before, want, mask.copy(), tags


CONFIGS = [("map1.txt", 5, 20, 25, 12),   # step_episode is one kernel
           ("map3.txt", 8, 80, 30, 12)]   # P > 64: the four-launch step_episode
# Random actions rarely deliver.  With these seeds the oracle alone (masked_run, no GPU) gives, over the
# int-ops run: map1 21 pickups, 5 deliveries, 59 wasted pickups; map3 52, 3 and 248.  Seed 77 delivers nothing.
SEEDS = {"map1.txt": 81, "map3.txt": 11}


def make_env(mg, cfg, tracker, seed):
    mapname, A, P, T, E = cfg
    env = mg.BatchedEnv(grid(mapname), E, A, P, T, seed=seed, tracker=tracker)
    # IDQ's trainer empties its tracker and then fills it from the reset state (IDQ/trainer.py:235-239):
    # a stale tracker is cleared BEFORE the reset.  Cleared after it, it would stay without the packages
    # that start at t = 0 (the update inserts a package at its start time only).
    if tracker != "fresh":
        env.clear_tracker()
    env.reset()
    return env


# ------------------------------------------------- 1. alt_transition along masked episodes
@pytest.mark.parametrize("ops_are_ints", [True, False], ids=["int-ops", "str-ops"])
@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}-A{c[1]}-P{c[2]}")
def test_alt_transition_vs_oracle_masked(cfg, tracker, ops_are_ints):
    import marl_gpu
    mapname, A, P, T, E = cfg
    seed = SEEDS[mapname]
    g = grid(mapname)
    H, W = g.shape
    env = make_env(marl_gpu, cfg, tracker, seed)
    run = masked_run(cfg, seed, 35, ops_are_ints)
    orc, mask0 = next(run)
    active = torch.from_numpy(mask0.astype(np.uint8)).cuda()
    filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
    pre = env.alt_pre_buffer()
    pre.fill_(0xA5)
    rows_pre = lambda p: p[:E * A * 16].reshape(E, A * 16)   # noqa: E731
    out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E, 7, H, W)))

    # begin form under the mask: no reward, the running envs' records and observations only
    r0, o0 = env.alt_transition(None, pre, row_mask=active, out=out, which=("idq_obs", "qmix_state"))
    assert r0 is None
    on, off = np.nonzero(mask0)[0], np.nonzero(~mask0)[0]
    assert off.size == E // 3
    p0 = pre.cpu().numpy()
    assert (rows_pre(p0)[off] == 0xA5).all() and (p0[E * A * 16:].view(np.int32)[off] == np.int32(-1515870811)).all()
    assert (p0[E * A * 16:].view(np.int32)[on] == 0).all()
    for k in ("idq_obs", "qmix_state"):
        assert (bits(o0[k])[off] == NAN_BITS).all(), f"begin: {k} rows of the masked envs were written"
    alt = env.build_obs_alt()
    for k in ("idq_obs", "qmix_state"):
        assert bits(o0[k])[on].tobytes() == bits(alt[k])[on].tobytes(), f"begin: {k} != build_obs_alt"
    for e in on:
        idq, qst = orc.obs(e, (7, H, W))
        np.testing.assert_array_equal(o0["idq_obs"][e].cpu().numpy(), idq)
        np.testing.assert_array_equal(o0["qmix_state"][e].cpu().numpy(), qst)

    total = dict(pickup=0, delivery=0, wasted=0)
    stepped = 0
    for k, (ints, before, want, after, tags) in enumerate(run):
        active.copy_(torch.from_numpy(before.astype(np.uint8)))
        acts = torch.from_numpy(ints).cuda()
        env.step_episode(acts, active, filled=filled, obs_out={}, which=())
        np.testing.assert_array_equal(filled.cpu().numpy().astype(bool), before, err_msg=f"step {k}: filled")
        np.testing.assert_array_equal(active.cpu().numpy().astype(bool), after, err_msg=f"step {k}: mask")
        pre_was = pre.cpu().numpy().copy()
        out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E, 7, H, W)))
        r, o = env.alt_transition(acts, pre, row_mask=filled, ops_are_ints=ops_are_ints, out=out,
                                  which=("idq_obs", "qmix_state"))
        r = r.cpu().numpy()
        idq, qst = o["idq_obs"].cpu().numpy(), o["qmix_state"].cpu().numpy()
        off = np.nonzero(~before)[0]
        assert not bits(r)[off].any(), f"step {k}: rewards of the unfilled envs are +0"
        assert (bits(idq)[off] == NAN_BITS).all() and (bits(qst)[off] == NAN_BITS).all(), f"step {k}: unfilled rows"
        pre_now = pre.cpu().numpy()
        assert rows_pre(pre_now)[off].tobytes() == rows_pre(pre_was)[off].tobytes(), f"step {k}: unfilled pre-record"
        assert pre_now[E * A * 16:].view(np.int32)[off].tobytes() == pre_was[E * A * 16:].view(np.int32)[off].tobytes()
        for e, (rw, iw, qw) in want.items():
            assert bits(r[e]).tobytes() == bits(rw).tobytes(), f"step {k} env {e}: r_idq {r[e]} != {rw}"
            np.testing.assert_array_equal(idq[e], iw, err_msg=f"step {k} env {e}: idq_obs")
            np.testing.assert_array_equal(qst[e], qw, err_msg=f"step {k} env {e}: qmix_state")
        if k in (0, 9) and want:
            alt = env.build_obs_alt()
            on = np.array(sorted(want))
            assert bits(idq)[on].tobytes() == bits(alt["idq_obs"])[on].tobytes(), f"step {k}: != build_obs_alt"
            assert bits(qst)[on].tobytes() == bits(alt["qmix_state"])[on].tobytes(), f"step {k}: != build_obs_alt"
        stepped += len(want)
        for kk in total:
            total[kk] += tags[kk]
    assert not active.cpu().numpy().any(), "every env passed its time limit and cleared its own mask byte"
    assert stepped > 0
    if ops_are_ints:   # not vacuous: the op branches of reward_shaping fired
        assert total["pickup"] >= 1 and total["delivery"] >= 1 and total["wasted"] >= 1, total
    env.close()


# ------------------------------------------------- 2. the general (non-fast) emit path
def test_alt_transition_general_path():
    import marl_gpu
    rs = np.random.RandomState(7 * 1000 + 9 * 10 + 4)
    H, W, A, P, T, E = 7, 9, 4, 12, 30, 6
    g = (rs.random_sample((H, W)) < 0.15).astype(np.uint8)
    g[0, :] = g[-1, :] = 1
    g[:, 0] = g[:, -1] = 1
    assert (H * W) % 4 != 0
    shape = (7, H + 3, W - 2)
    env = marl_gpu.BatchedEnv(g, E, A, P, T, seed=31, tracker="fresh")
    env.reset()
    orc = OracleEpisodes(g, E, A, P, T, 31)
    pre = env.alt_pre_buffer()
    active = torch.ones(E, dtype=torch.uint8, device="cuda")
    active[2] = 0
    filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
    env.alt_transition(None, pre)
    for k in range(10):
        ints = rs.randint(0, 15, size=(E, A)).astype(np.uint8)
        acts = torch.from_numpy(ints).cuda()
        env.step_episode(acts, active, filled=filled, obs_out={}, which=())
        out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E,) + shape))
        r, o = env.alt_transition(acts, pre, row_mask=filled, ops_are_ints=True, out=out, state_shape=shape,
                                  which=("idq_obs", "qmix_state"))
        r = r.cpu().numpy()
        for e in range(E):
            if e == 2:
                assert not bits(r[e]).any()
                assert (bits(o["idq_obs"][e]) == NAN_BITS).all() and (bits(o["qmix_state"][e]) == NAN_BITS).all()
                continue
            rw, _, _ = orc.step(e, ints[e], True)
            iw, qw = orc.obs(e, shape)
            assert bits(r[e]).tobytes() == bits(rw).tobytes(), f"step {k} env {e}: r_idq {r[e]} != {rw}"
            np.testing.assert_array_equal(o["idq_obs"][e].cpu().numpy(), iw, err_msg=f"step {k} env {e}")
            np.testing.assert_array_equal(o["qmix_state"][e].cpu().numpy(), qw, err_msg=f"step {k} env {e}")
    env.close()


# ------------------------------------------------- 4. the replay append
class NumpyRing:
    """ReplayBuffer (IDQ/networks.py:46-79): the literal sequential add."""

    def __init__(self, capacity, obs_shape):
        self.capacity = capacity
        self.observations = np.zeros((capacity,) + obs_shape, np.float32)
        self.actions = np.zeros(capacity, np.int64)
        self.rewards = np.zeros(capacity, np.float32)
        self.next_observations = np.zeros((capacity,) + obs_shape, np.float32)
        self.dones = np.zeros(capacity, np.bool_)
        self.ptr = self.size = 0

    def add(self, obs, action, reward, next_obs, done):
        self.observations[self.ptr] = obs
        self.actions[self.ptr] = action
        self.rewards[self.ptr] = reward
        self.next_observations[self.ptr] = next_obs
        self.dones[self.ptr] = done
        self.ptr = (self.ptr + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def add_step(self, filled, obs, actions, reward, next_obs, done):
        """IDQ/trainer.py:286-311 for one step: env order, then agent order."""
        for e in range(filled.shape[0]):
            if not filled[e]:
                continue
            for a in range(actions.shape[1]):
                self.add(obs[e, a], int(actions[e, a]), reward[e, a], next_obs[e, a], bool(done[e]))


def assert_ring_equal(rep, ref, what):
    assert rep.position() == (ref.ptr, ref.size), f"{what}: cursor {rep.position()} != {(ref.ptr, ref.size)}"
    assert bits(rep.observations).tobytes() == bits(ref.observations).tobytes(), f"{what}: observations"
    assert bits(rep.next_observations).tobytes() == bits(ref.next_observations).tobytes(), f"{what}: next_observations"
    np.testing.assert_array_equal(rep.actions.cpu().numpy(), ref.actions, err_msg=f"{what}: actions")
    assert bits(rep.rewards).tobytes() == bits(ref.rewards).tobytes(), f"{what}: rewards"
    np.testing.assert_array_equal(rep.dones.cpu().numpy().astype(bool), ref.dones, err_msg=f"{what}: dones")


@pytest.mark.parametrize("capacity", [64, 31, 20])
@pytest.mark.parametrize("row", [6, 8], ids=["scalar-rows", "vector-rows"])
def test_replay_append_vs_sequential_adds(row, capacity):
    from marl_gpu.idq_rollout import TransitionReplay
    E, A = 9, 3
    rep = TransitionReplay(capacity, (row,), device="cuda")
    ref = NumpyRing(capacity, (row,))
    rs = np.random.RandomState(row * 100 + capacity)
    for k in range(12):
        filled = (rs.rand(E) < 0.6).astype(np.uint8)
        if k == 3:
            filled[:] = 0
        if k in (5, 6):      # two full steps in a row: 27 rows each
            filled[:] = 1
        # distinct values per (step, env, agent, column): a misplaced row cannot compare equal
        ids = (k * E * A + np.arange(E * A).reshape(E, A)).astype(np.float64)
        obs = (ids[..., None] * 16 + np.arange(row)).astype(np.float32)
        nxt = obs + np.float32(0.5)
        reward = ids * 0.1 + 1e-9                 # not float32 values: the append rounds once
        actions = ((ids.astype(np.int64) * 7) % 251).astype(np.uint8)
        done = (rs.rand(E) < 0.3).astype(np.uint8)
        rep.add(*(torch.from_numpy(x).cuda() for x in (filled, obs, actions, reward, nxt, done)))
        ref.add_step(filled, obs, actions, reward, nxt, done)
        assert_ring_equal(rep, ref, f"row {row} capacity {capacity} step {k}")
    assert ref.size == capacity


def test_replay_append_unaligned_rows_take_the_scalar_path():
    """Rows of 8 floats from a tensor whose storage starts 4 bytes off a 16-byte boundary."""
    from marl_gpu.idq_rollout import TransitionReplay
    E, A, row, capacity = 9, 3, 8, 31
    rep = TransitionReplay(capacity, (row,), device="cuda")
    ref = NumpyRing(capacity, (row,))
    rs = np.random.RandomState(5)
    for k in range(3):
        filled = (rs.rand(E) < 0.7).astype(np.uint8)
        obs = rs.rand(E, A, row).astype(np.float32)
        nxt = rs.rand(E, A, row).astype(np.float32)
        reward = rs.rand(E, A)
        actions = rs.randint(0, 15, size=(E, A)).astype(np.uint8)
        done = (rs.rand(E) < 0.3).astype(np.uint8)
        od = torch.zeros(E * A * row + 1, dtype=torch.float32, device="cuda")[1:].view(E, A, row)
        od.copy_(torch.from_numpy(obs))
        assert od.data_ptr() % 16 == 4 and od.is_contiguous()
        rep.add(torch.from_numpy(filled).cuda(), od, torch.from_numpy(actions).cuda(), torch.from_numpy(reward).cuda(),
                torch.from_numpy(nxt).cuda(), torch.from_numpy(done).cuda())
        ref.add_step(filled, obs, actions, reward, nxt, done)
        assert_ring_equal(rep, ref, f"step {k}")


def test_replay_append_refuses_too_many_envs():
    import marl_gpu
    from marl_gpu import _lib
    from marl_gpu.idq_rollout import TransitionReplay
    E = _lib.MDL_REPLAY_MAX_ENVS + 1
    rep = TransitionReplay(8, (4,), device="cuda")
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device="cuda")   # noqa: E731
    with pytest.raises(marl_gpu.MdlError, match="MDL_REPLAY_MAX_ENVS"):
        rep.add(z(E), z(E, 1, 4, dt=torch.float32), z(E, 1), z(E, 1, dt=torch.float64), z(E, 1, 4, dt=torch.float32), z(E))
    assert rep.position() == (0, 0)


# ------------------------------------------------- 5. / 6. the collector
COLLECT = dict(cfg=("map1.txt", 5, 20, 12, 8), eps=0.3, env_seed=300, agent_seed=5, seed=13, capacity=301)


def make_agent(H, W):
    """A small fixed-weight linear Q network on the flattened observation."""
    lin = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(6 * H * W, 15))
    g = torch.Generator().manual_seed(COLLECT["agent_seed"])
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return lin.cuda()


def make_collector(mg, tracker="fresh", ops_are_ints=True):
    from marl_gpu.idq_rollout import IdqCollector, TransitionReplay
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    env = mg.BatchedEnv(grid(mapname), E, A, P, T, seed=c["env_seed"], tracker=tracker)
    H, W = grid(mapname).shape
    rep = TransitionReplay(c["capacity"], (6, H, W), device="cuda")
    return env, rep, IdqCollector(env, rep, seed=c["seed"], ops_are_ints=ops_are_ints)


def test_collector_equals_hand_written_loop():
    import marl_gpu
    from marl_gpu.idq_rollout import select_actions_eps
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    H, W = grid(mapname).shape
    env, rep, col = make_collector(marl_gpu)
    agent = make_agent(H, W)
    agent.train()
    ret1 = col.collect(agent, c["eps"]).clone()
    assert agent.training                                       # the mode is restored
    ret2 = col.collect(agent, c["eps"], max_steps=5).clone()    # a second, cut episode: the ring wraps
    assert col.offset == T + 5

    ref = marl_gpu.BatchedEnv(grid(mapname), E, A, P, T, seed=c["env_seed"], tracker="fresh")
    ring = NumpyRing(c["capacity"], (6, H, W))
    agent.eval()
    obs = torch.zeros((2, E, A, 6, H, W), dtype=torch.float32, device="cuda")
    pre = ref.alt_pre_buffer()
    active = torch.zeros(E, dtype=torch.uint8, device="cuda")
    filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
    u = torch.zeros((E, A), dtype=torch.uint8, device="cuda")
    offset, lengths = 0, []
    with torch.no_grad():
        for n_steps in (T, 5):
            ref.reset()
            active.fill_(1)
            ref.alt_transition(None, pre, out={"idq_obs": obs[0]})
            cur, length = 0, np.zeros(E, np.int64)
            for _ in range(n_steps):
                q = agent(obs[cur].reshape(E * A, 6, H, W))
                select_actions_eps(q, c["eps"], c["seed"], offset, out=u.view(-1))
                offset += 1
                _, _, done, _ = ref.step_episode(u, active, filled=filled, obs_out={}, which=())
                r, _ = ref.alt_transition(u, pre, row_mask=filled, ops_are_ints=True, out={"idq_obs": obs[1 - cur]})
                ring.add_step(filled.cpu().numpy(), obs[cur].cpu().numpy(), u.cpu().numpy(), r.cpu().numpy(),
                              obs[1 - cur].cpu().numpy(), done.cpu().numpy())
                length += filled.cpu().numpy()
                cur = 1 - cur
            lengths.append(length)
            got = ret1 if n_steps == T else ret2
            assert bits(got).tobytes() == bits(ref.read_state()["total_reward"]).tobytes(), "episode_return"
    assert_ring_equal(rep, ring, "collector vs hand-written loop")
    assert ring.size == c["capacity"] and int(lengths[0].sum() + lengths[1].sum()) * A > c["capacity"]
    assert bits(col.episode_return).tobytes() == bits(ref.read_state()["total_reward"]).tobytes()
    np.testing.assert_array_equal(env.read_state()["t"].cpu().numpy(), lengths[1])
    assert len(set(ring.rewards.tolist())) > 3, "the rewards must vary"
    env.close()
    ref.close()


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
def test_collector_graph_replay_equals_eager(tracker):
    import marl_gpu
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    H, W = grid(mapname).shape
    env_e, rep_e, eager = make_collector(marl_gpu, tracker)
    env_g, rep_g, graph = make_collector(marl_gpu, tracker)
    agent = make_agent(H, W)
    for call, eps in enumerate((c["eps"], 0.5, 0.1)):   # the later graph calls are replays, at other epsilons
        x = eager.collect(agent, eps).clone()
        y = graph.collect(agent, eps, graph=True).clone()
        assert bits(x).tobytes() == bits(y).tobytes(), f"call {call}: episode_return"
        assert rep_e.position() == rep_g.position(), f"call {call}: cursor"
        for k in ("observations", "next_observations", "actions", "rewards", "dones"):
            assert bits(getattr(rep_e, k)).tobytes() == bits(getattr(rep_g, k)).tobytes(), f"call {call}: {k}"
        assert env_e.save_state().tobytes() == env_g.save_state().tobytes()
        assert eager.offset == graph.offset == (call + 1) * T and eager.cur == graph.cur
    assert graph.captured_graphs() == {None: T}
    assert rep_e.position()[1] == c["capacity"]
    env_e.close()
    env_g.close()


def test_graph_and_eager_collects_interleave():
    """Graphed and eager ``collect`` calls on one collector, and an assigned ``offset``, select exactly
    what eager calls alone select: the host offset is written to the device before every replay."""
    import marl_gpu
    from marl_gpu.idq_rollout import IdqCollector, TransitionReplay
    c = COLLECT
    E, A, P, T, n, eps = 4, 2, 2, 20, 4, 0.5   # epsilon 0.5: about half the rows' actions depend on the offset
    H, W = grid("map.txt").shape

    def make():
        env = marl_gpu.BatchedEnv(grid("map.txt"), E, A, P, T, seed=c["env_seed"], tracker="fresh")
        rep = TransitionReplay(29, (6, H, W), device="cuda")   # the ring wraps during the sequence
        return env, rep, IdqCollector(env, rep, seed=c["seed"], ops_are_ints=True)

    env_e, rep_e, eager = make()
    env_o, rep_o, other = make()
    agent = make_agent(H, W)
    for call, graph in enumerate((True, True, False, True, True)):   # capture, replay, eager, replay, replay
        if call == 4:
            other.offset = eager.offset = 1000
        x = eager.collect(agent, eps, max_steps=n).clone()
        y = other.collect(agent, eps, max_steps=n, graph=graph).clone()
        assert bits(x).tobytes() == bits(y).tobytes(), f"call {call}: episode_return"
        assert rep_e.position() == rep_o.position(), f"call {call}: cursor"
        for k in ("observations", "next_observations", "actions", "rewards", "dones"):
            assert bits(getattr(rep_e, k)).tobytes() == bits(getattr(rep_o, k)).tobytes(), f"call {call}: {k}"
        for k in ("obs", "u", "r_idq", "r_env", "done", "filled", "active"):
            assert bits(getattr(eager, k)).tobytes() == bits(getattr(other, k)).tobytes(), f"call {call}: {k}"
        assert env_e.save_state().tobytes() == env_o.save_state().tobytes(), f"call {call}"
        assert eager.offset == other.offset == (1000 + n if call == 4 else (call + 1) * n), f"call {call}"
        assert eager.cur == other.cur
    assert other.captured_graphs() == {None: n}
    env_e.close()
    env_o.close()
