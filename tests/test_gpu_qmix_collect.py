"""Device-resident QMIX episode collection: the masked step + observation launch
(``BatchedEnv.step_episode``) against the reference-generated QMIX fixture and against the
host-driven subset loop (``step(env_ids=...)`` + ``build_obs``), the epsilon-greedy selection
kernel against its numpy restatement, and ``QmixCollector`` against a hand-written loop and
against its own hipGraph replay.  Everything is compared bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from golden_io import grid, meta, npz  # noqa: E402

OBS_KEYS = ("actor_map", "actor_vec", "critic_map", "critic_vec")
SENTINEL = -7.25   # no observation feature is negative


def _mg():
    import marl_gpu
    import marl_gpu.qmix_rollout as Q
    return marl_gpu, Q


def bits(t):
    """Bit pattern of a float tensor as a numpy integer array (exact comparison, -0.0 != 0.0)."""
    a = t.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---------------------------------------------------------------- 1. fixture replay
def test_step_episode_replays_qmix_fixture():
    mg, _ = _mg()
    d = npz("rollout_qmix.npz")
    m = meta(d)
    E, A, P, T = m["E"], m["A"], m["P"], m["T"]
    env = mg.BatchedEnv(grid(m["map"]), E, A, P, T, seed=m["seed"], tracker="fresh", shaping="qmix",
                        max_other_robots=m["MO"], max_packages_obs=m["MP"], max_robots_state=m["MR"],
                        max_packages_state=m["MPs"])
    env.reset()
    active = torch.ones(E, dtype=torch.uint8, device="cuda")
    filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
    steps = resets = 0
    for k in range(d["active"].shape[0]):
        if not d["active"][k].any():   # the fixture's reset between its two iterations
            assert not active.cpu().numpy().any(), f"active after the episode's last step (row {k})"
            env.reset()
            active.fill_(1)
            o = env.build_obs()
            resets += 1
        else:
            assert d["active"][k].all()   # in this fixture the envs end only together, at t = T
            a = torch.from_numpy(d["acts"][k].astype(np.uint8)).cuda()
            r, sh, dn, o = env.step_episode(a, active, filled=filled)
            assert r.cpu().numpy().tobytes() == d["r"][k].astype(np.float64).tobytes(), f"r row {k}"
            assert sh.cpu().numpy().tobytes() == d["sh"][k].astype(np.float32).tobytes(), f"shaped row {k}"
            np.testing.assert_array_equal(dn.cpu().numpy().astype(bool), d["done"][k], err_msg=f"done row {k}")
            assert filled.cpu().numpy().all()
            np.testing.assert_array_equal(active.cpu().numpy().astype(bool), ~d["done"][k].astype(bool))
            steps += 1
        o = {kk: v.cpu().numpy() for kk, v in o.items()}
        np.testing.assert_array_equal(o["actor_vec"], d["avec"][k], err_msg=f"avec row {k}")
        np.testing.assert_array_equal(o["critic_vec"], d["cvec"][k], err_msg=f"cvec row {k}")
        np.testing.assert_array_equal(o["actor_map"], d["amap"][k], err_msg=f"amap row {k}")
    assert steps == 2 * T and resets >= 1
    if d["active"][-1].any():   # the fixture ends on a step row: all zero after the last iteration too
        assert not active.cpu().numpy().any()
    else:                       # it ends on a reset row, which checked the mask before re-arming it
        assert resets == 2
    env.close()


# ------------------------------------------- 2. masked launch == host-driven subset loop
GREEDY_LENGTHS = {   # CPU oracle, seeds 42 + e
    "map.txt": [60, 60, 8, 60, 7, 60, 60, 60, 60, 60, 60, 60, 8, 6, 60, 9],
    "map1.txt": [10, 60, 60, 9, 60, 11, 60, 6, 60, 60, 60, 10, 7, 11, 60, 10],
}
CASES = [   # map, A, P, T, E, greedy actions
    ("map.txt", 3, 2, 60, 16, True),     # the fused launch
    ("map1.txt", 9, 2, 60, 16, True),    # A > 8: the composed launches
    ("map1.txt", 8, 64, 12, 13, False),  # the fused launch's edge; E no multiple of the waves per block
    ("map1.txt", 5, 65, 12, 8, False),   # two package chunks: composed
]


class _Pair:
    """One engine stepped by step_episode, its twin by the parent's subset step + build_obs."""

    def __init__(self, mg, case, tracker):
        mapname, A, P, T, E, greedy = case
        kw = dict(seed=42, tracker=tracker, shaping="qmix")
        self.a = mg.BatchedEnv(grid(mapname), E, A, P, T, **kw)
        self.b = mg.BatchedEnv(grid(mapname), E, A, P, T, **kw)
        self.E, self.fmt = E, "codes" if greedy else "int"
        for env in (self.a, self.b):
            env.reset()
            if tracker != "fresh":
                env.clear_tracker()
            if greedy:
                env.greedy_init()
        self.obs_a = self.a.obs_buffers()
        self.out = (torch.zeros(E, dtype=torch.float64, device="cuda"), torch.zeros(E, dtype=torch.float32, device="cuda"),
                    torch.zeros(E, dtype=torch.uint8, device="cuda"))
        self.filled = torch.zeros(E, dtype=torch.uint8, device="cuda")

    def step(self, acts, mask_h, what):
        """One masked transition on both engines; returns the mask the device left and done."""
        E = self.E
        mask = torch.from_numpy(mask_h.astype(np.uint8)).cuda()
        for v in self.obs_a.values():
            v.fill_(SENTINEL)
        self.out[0].fill_(float("nan"))
        self.out[1].fill_(float("nan"))
        self.out[2].fill_(9)
        self.filled.fill_(9)
        r, sh, dn, oa = self.a.step_episode(acts, mask, action_format=self.fmt, out=self.out, filled=self.filled,
                                            obs_out=self.obs_a)
        idx = np.nonzero(mask_h)[0]
        done_b = np.zeros(E, bool)
        if idx.size:
            rb, shb, dnb = self.b.step(acts[torch.from_numpy(idx).cuda()].contiguous(), env_ids=idx.tolist(),
                                       auto_reset=False, action_format=self.fmt)
            assert bits(r)[idx].tobytes() == bits(rb).tobytes(), f"{what}: fp64 reward bits"
            assert bits(sh)[idx].tobytes() == bits(shb).tobytes(), f"{what}: shaped reward bits"
            done_b[idx] = dnb.cpu().numpy().astype(bool)
        ob = self.b.build_obs()
        assert self.a.save_state().tobytes() == self.b.save_state().tobytes(), f"{what}: engine state"
        np.testing.assert_array_equal(dn.cpu().numpy().astype(bool), done_b, err_msg=f"{what}: done")
        np.testing.assert_array_equal(self.filled.cpu().numpy(), mask_h.astype(np.uint8), err_msg=f"{what}: filled")
        off = np.nonzero(~mask_h.astype(bool))[0]
        assert not bits(r)[off].any() and not bits(sh)[off].any(), f"{what}: inactive rewards are +0"
        for k in OBS_KEYS:
            xa, xb = bits(oa[k]), bits(ob[k])
            assert xa[idx].tobytes() == xb[idx].tobytes(), f"{what}: {k} rows of the stepped envs"
            sent = np.float32(SENTINEL).view(np.uint32)
            assert (xa[off] == sent).all(), f"{what}: {k} rows of the inactive envs were written"
        left = mask.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(left, mask_h.astype(bool) & ~done_b, err_msg=f"{what}: mask after the step")
        return left, done_b


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-A{c[1]}-P{c[2]}-E{c[4]}")
def test_step_episode_equals_host_loop(case, tracker):
    mg, _ = _mg()
    mapname, A, P, T, E, greedy = case
    pair = _Pair(mg, case, tracker)
    rs = np.random.RandomState(7)
    mask = np.ones(E, bool)
    length = np.zeros(E, np.int64)
    ended = np.zeros(E, bool)   # by the env (done), not cut by the test
    for k in range(T):
        if greedy:
            acts = pair.a.greedy_actions()
            assert torch.equal(acts, pair.b.greedy_actions())
        else:
            acts = torch.from_numpy(rs.randint(0, 15, size=(E, A)).astype(np.uint8)).cuda()
        if k == 3:
            mask[1] = False   # an episode cut by the caller
        if not greedy and k >= 2:
            keep = rs.rand(E) > 0.06
            keep[E - 1] |= k <= 4   # the last env runs at least until the split step below
            mask &= keep
        length += mask
        if k == 4:   # this step in three calls: an all-zero mask, only the last env, then the rest
            assert mask[E - 1]
            left, _ = pair.step(acts, np.zeros(E, bool), f"step {k} all-zero mask")
            assert not left.any()
            only_last = np.zeros(E, bool)
            only_last[E - 1] = True
            left_l, dn_l = pair.step(acts, only_last, f"step {k} last env only")
            rest = mask.copy()
            rest[E - 1] = False
            mask, dn = pair.step(acts, rest, f"step {k} all but the last env")
            mask[E - 1] = left_l[E - 1]
            ended |= dn | dn_l
            continue
        mask, dn = pair.step(acts, mask.copy(), f"step {k}")
        ended |= dn
    assert ended.any() and not mask.any()
    if greedy:
        want = np.array(GREEDY_LENGTHS[mapname])
        np.testing.assert_array_equal(length[ended], want[ended])
        assert len(set(length[ended].tolist())) >= 3, "the inputs must end episodes at different times"
    pair.a.close()
    pair.b.close()


# ---------------------------------------------------------------- 3. selection
def philox4(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy arrays: all four output words (tests/test_gpu_rollout.py's restatement)."""
    c = [np.asarray(x, np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return [x.astype(np.uint32) for x in c]


def ref_select(q, avail, eps, seed, offset):
    """include/mdl_engine.h's statement of mdl_select_actions_eps, in numpy."""
    N, K = q.shape
    rows = np.arange(N, dtype=np.uint64)
    z = np.zeros(N, np.uint64)
    x0, x1, _, _ = philox4(z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64(offset >> 32), rows & np.uint64(0xFFFFFFFF),
                           rows >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    u = (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    explore = u < np.float32(eps)
    n_avail = avail.sum(1).astype(np.uint64)
    kth = ((x1.astype(np.uint64) * n_avail) >> np.uint64(32)).astype(np.int64)
    rank = np.cumsum(avail, axis=1) - 1                      # index among the available actions
    rand = np.argmax(avail & (rank == kth[:, None]), axis=1)
    best = np.full(N, -1)
    qb = np.zeros(N, np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(K):
            v = q[:, i]
            take = avail[:, i] & ((best < 0) | (v > qb) | (np.isnan(qb) & ~np.isnan(v)))
            best = np.where(take, i, best)
            qb = np.where(take, v, qb)
    greedy = np.where(best < 0, 0, best)
    return np.where(explore & (n_avail > 0), rand, greedy).astype(np.uint8), explore


def _selection_inputs(N, K=15, seed=0):
    rs = np.random.RandomState(seed)
    q = rs.randn(N, K).astype(np.float32)
    avail = rs.rand(N, K) < 0.6
    avail[0:64] = False                                       # rows with no available action
    avail[64:128] = False
    avail[np.arange(64, 128), rs.randint(0, K, 64)] = True    # rows with exactly one
    q[128:192, 3] = q[128:192, 9] = q[128:192, 12] = 5.0      # constructed ties at the maximum
    avail[128:192, 9] = True
    q[192:256] = -np.inf                                      # rows holding only -inf ...
    q[256:320, ::2] = -np.inf                                 # ... and some -inf
    q[320:336, 0] = np.nan                                    # a NaN never wins over a number
    avail[320:336, 0] = True
    avail[320:336, 5] = True
    return q, avail


def test_select_actions_eps_matches_restatement():
    _, Q = _mg()
    N, K = 4096, 15
    q, avail = _selection_inputs(N)
    seed, off = 0x0123_4567_89AB_CDEF, (5 << 32) + 11
    qd, ad = torch.from_numpy(q).cuda(), torch.from_numpy(avail).cuda()
    got = Q.select_actions_eps(qd, 0.3, seed, off, avail=ad).cpu().numpy()
    want, explore = ref_select(q, avail, 0.3, seed, off)
    np.testing.assert_array_equal(got, want)
    assert 0 < explore.sum() < N
    assert (got[:64] == 0).all()                                               # no available action -> 0
    has = avail.any(1)
    assert avail[np.nonzero(has)[0], got[has]].all()                            # never an unavailable action

    # epsilon = 0: the masked first-index argmax (a row whose available q are all -inf: its first available action)
    g0 = Q.select_actions_eps(qd, 0.0, seed, off, avail=ad).cpu().numpy()
    ok = ~np.isnan(q).any(1)
    qm = np.where(avail, q, -np.inf)
    arg = np.argmax(qm, axis=1)
    arg = np.where(np.isneginf(qm.max(1)), np.argmax(avail, axis=1), arg)
    np.testing.assert_array_equal(g0[ok], arg[ok].astype(np.uint8))
    np.testing.assert_array_equal(g0[128:192], np.where(avail[128:192, 3], 3, 9))   # ties: the lowest available index
    assert (g0[320:336] != 0).all()                                             # the NaN rows
    # epsilon = 1 explores every row; no mask = every action available
    g1 = Q.select_actions_eps(qd, 1.0, seed, off, avail=ad).cpu().numpy()
    w1, e1 = ref_select(q, avail, 1.0, seed, off)
    assert e1.all()
    np.testing.assert_array_equal(g1, w1)
    gn = Q.select_actions_eps(qd, 0.3, seed, off).cpu().numpy()
    np.testing.assert_array_equal(gn, ref_select(q, np.ones_like(avail), 0.3, seed, off)[0])

    # independent of the launch shape: the same rows inside a 65,536-row call
    big_q, big_a = _selection_inputs(65536, seed=1)
    big_q[:N], big_a[:N] = q, avail
    gb = Q.select_actions_eps(torch.from_numpy(big_q).cuda(), 0.3, seed, off, avail=torch.from_numpy(big_a).cuda())
    np.testing.assert_array_equal(gb.cpu().numpy()[:N], got)

    # the device-argument form at the same values
    eps_dev = torch.tensor([0.3], dtype=torch.float32, device="cuda")
    base = off - 1000
    off_dev = torch.tensor([base], dtype=torch.int64, device="cuda")
    gd = Q.select_actions_eps_dev(qd, eps_dev, seed, off_dev, 1000, avail=ad)
    np.testing.assert_array_equal(gd.cpu().numpy(), got)


def test_select_actions_eps_frequencies():
    _, Q = _mg()
    N, K, eps = 65536, 15, 0.25
    q = np.zeros((N, K), np.float32)
    q[:, 7] = 1.0   # the greedy action of every row
    seed, off = 99, 3
    got = Q.select_actions_eps(torch.from_numpy(q).cuda(), eps, seed, off).cpu().numpy()
    _, explore = ref_select(q, np.ones((N, K), bool), eps, seed, off)
    assert (got[~explore] == 7).all()
    n = int(explore.sum())
    sd = np.sqrt(N * eps * (1 - eps))                          # ~ 111
    assert abs(n - N * eps) <= 6 * sd, (n, N * eps, sd)
    p = 1.0 / K
    sd_a = np.sqrt(n * p * (1 - p))
    counts = np.bincount(got[explore], minlength=K)
    assert (np.abs(counts - n * p) <= 6 * sd_a).all(), counts


# ---------------------------------------------------------------- 4. collector
HD = 16
# The seeds are chosen so that the run holds episodes of different lengths: with them env 3 delivers both
# packages at step 21 and the other envs run to T (the collector's actions replayed through the CPU
# oracle, seeds 200 + e, give these lengths and the same fp64 returns).  Most seeds end every episode at T.
COLLECT = dict(mapname="map.txt", A=3, P=2, T=60, E=16, eps=0.2, env_seed=200, agent_seed=35, seed=11)
BATCH_KEYS = ("so", "vo", "gs", "gv", "u", "r", "r64", "r_shaped", "terminated", "filled", "hidden", "episode_return",
              "episode_length")


def make_agent(dv):
    """A small fixed-weight recurrent agent: linear layer on vo, GRUCell, linear Q head; weights
    generated on the CPU from a fixed seed."""
    nn = torch.nn

    class Agent(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(dv, HD)
            self.rnn = nn.GRUCell(HD, HD)
            self.out = nn.Linear(HD, 15)

        def init_hidden(self):
            return self.fc.weight.new_zeros(1, HD)

        def forward(self, so, vo, h):
            h = self.rnn(torch.relu(self.fc(vo)), h)
            return self.out(h), h

    a = Agent()
    g = torch.Generator().manual_seed(COLLECT["agent_seed"])
    with torch.no_grad():
        for p in a.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return a.cuda()


def make_env(mg, tracker="fresh"):
    c = COLLECT
    return mg.BatchedEnv(grid(c["mapname"]), c["E"], c["A"], c["P"], c["T"], seed=c["env_seed"], tracker=tracker,
                         shaping="qmix")


def snapshot(batch):
    return {k: batch[k].clone() for k in BATCH_KEYS}


def assert_batches_equal(x, y, what):
    for k in BATCH_KEYS:
        assert bits(x[k]).tobytes() == bits(y[k]).tobytes(), f"{what}: {k}"


def test_collector_equals_hand_written_loop():
    mg, Q = _mg()
    c = COLLECT
    E, A, L = c["E"], c["A"], c["T"]
    env = make_env(mg)
    agent = make_agent(env.actor_vec_dim)
    agent.train()
    col = Q.QmixCollector(env, episode_limit=100, seed=c["seed"])   # L = min(100, T)
    assert col.L == L
    b = col.collect(agent, c["eps"])
    assert agent.training                                           # the mode is restored
    torch.cuda.synchronize()

    # the same episode by hand: select_actions_eps + step_episode at the same seed and offsets
    ref = make_env(mg)
    hand = Q.QmixCollector(ref, episode_limit=100, seed=c["seed"])  # only its (zeroed) buffers are used
    ref.reset()
    active = torch.ones(E, dtype=torch.uint8, device="cuda")
    ref.build_obs(out=hand._slot(0))
    h = agent.init_hidden().expand(E * A, -1)
    agent.eval()
    with torch.no_grad():
        for t in range(L):
            q, h = agent(hand.so[t].reshape(E * A, *hand.so.shape[3:]), hand.vo[t].reshape(E * A, -1), h)
            Q.select_actions_eps(q, c["eps"], c["seed"], t, out=hand.u[t].view(-1))
            ref.step_episode(hand.u[t], active, out=(hand.r64[t], hand.r_shaped[t], hand.terminated[t]),
                             filled=hand.filled[t], obs_out=hand._slot(t + 1))
    for k in ("so", "vo", "gs", "gv", "u", "r64", "r_shaped", "terminated", "filled"):
        assert bits(b[k]).tobytes() == bits(getattr(hand, k)).tobytes(), k
    assert bits(b["r"]).tobytes() == bits(hand.r64.float()).tobytes()
    assert bits(b["hidden"]).tobytes() == bits(h).tobytes()

    st = env.read_state()
    assert bits(b["episode_return"]).tobytes() == bits(st["total_reward"]).tobytes()
    filled = b["filled"].cpu().numpy()
    length = filled.sum(0)
    np.testing.assert_array_equal(b["episode_length"].cpu().numpy(), length)
    np.testing.assert_array_equal(st["t"].cpu().numpy(), length)
    assert (np.diff(filled.astype(np.int8), axis=0) <= 0).all()     # filled is a prefix of every column
    term = b["terminated"].cpu().numpy()
    for e in range(E):
        if length[e] < L:   # ended by the env before the limit: terminated exactly at its last filled step
            want = np.zeros(L, np.uint8)
            want[length[e] - 1] = 1
            np.testing.assert_array_equal(term[:, e], want, err_msg=f"env {e}")
    assert len(set(length.tolist())) >= 2, f"the run must hold episodes of different lengths: {length.tolist()}"
    assert col.offset == L
    env.close()
    ref.close()


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
def test_collector_graph_replay_equals_eager(tracker):
    mg, Q = _mg()
    c = COLLECT
    env_e, env_g = make_env(mg, tracker), make_env(mg, tracker)
    agent = make_agent(env_e.actor_vec_dim)
    eager = Q.QmixCollector(env_e, c["T"], seed=c["seed"])
    graph = Q.QmixCollector(env_g, c["T"], seed=c["seed"])
    for call, eps in enumerate((c["eps"], 0.35)):   # the second graph call is a replay, at another epsilon
        x = snapshot(eager.collect(agent, eps))
        y = snapshot(graph.collect(agent, eps, graph=True))
        assert_batches_equal(x, y, f"call {call}")
        assert env_e.save_state().tobytes() == env_g.save_state().tobytes()
        assert eager.offset == graph.offset == (call + 1) * c["T"]
    assert graph.captured_graphs() == {None: c["T"]}
    env_e.close()
    env_g.close()


def test_graph_and_eager_collects_interleave():
    """Graphed and eager ``collect`` calls on one collector, and an assigned ``offset``, select exactly
    what eager calls alone select: the host offset is written to the device before every replay."""
    mg, Q = _mg()
    E, A, P, T, L, eps = 4, 2, 2, 20, 4, 0.5   # epsilon 0.5: about half the rows' actions depend on the offset

    def make():
        return mg.BatchedEnv(grid("map.txt"), E, A, P, T, seed=COLLECT["env_seed"], tracker="fresh", shaping="qmix")

    env_e, env_o = make(), make()
    agent = make_agent(env_e.actor_vec_dim)
    eager, other = Q.QmixCollector(env_e, L, seed=COLLECT["seed"]), Q.QmixCollector(env_o, L, seed=COLLECT["seed"])
    for call, graph in enumerate((True, True, False, True, True)):   # capture, replay, eager, replay, replay
        if call == 4:
            other.offset = eager.offset = 1000
        x = snapshot(eager.collect(agent, eps))
        y = snapshot(other.collect(agent, eps, graph=graph))
        assert_batches_equal(x, y, f"call {call}")
        assert env_e.save_state().tobytes() == env_o.save_state().tobytes(), f"call {call}"
        assert eager.offset == other.offset == (1000 + L if call == 4 else (call + 1) * L), f"call {call}"
    assert other.captured_graphs() == {None: L}
    env_e.close()
    env_o.close()
