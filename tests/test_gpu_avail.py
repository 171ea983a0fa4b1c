"""The valid-action mask on the device: ``BatchedEnv.avail_actions`` against the numpy rule
(tests/avail_ref.py, itself pinned against ``env.step`` in tests/test_avail_cpu.py) on ``read_state``,
bit for bit, along greedy-plus-random rollouts of every shape class the kernel serves; its ``active``
argument; the masked sampler against its numpy restatement and the unmasked sampler; and the loops
that take the mask (``QmixCollector``, ``EpisodeReplay``, ``Evaluator``, ``MappoRollout``) against
hand-written loops, their own hipGraph replays and their unmasked selves."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import avail_ref as R  # noqa: E402
from golden_io import TRAINER_MOVE_CODES, grid  # noqa: E402

MIXED = ["map2.txt", "map3.txt", "map4.txt", "map5.txt"]
CASES = {   # maps, A, P, E, steps compared
    "walls": (["map.txt"], 3, 6, 8, 20),            # 7x7: borders and walls on nearly every robot
    "blocks": (["map1.txt"], 5, 50, 67, 16),        # a last workgroup with one wave past E, several XCD slots
    "chunks": (["map1.txt"], 5, 100, 9, 16),        # two package chunks, the README evaluation shape
    "wide": (["synthetic64.txt"], 16, 100, 5, 12),  # 5 * A > 64, a 4096-cell map
    "robots": (["map2.txt"], 40, 20, 3, 12),        # many robots, few packages
    "mixed": (MIXED, 5, 30, 8, 16),                 # the per-env map (one 20x20 shape)
}
RUNS = [(c, "fresh") for c in CASES] + [("blocks", "mappo"), ("wide", "mappo")]
T_LONG = 200                       # no episode ends within the steps compared


def _mg():
    import marl_gpu
    return marl_gpu


def _make(case, tracker="fresh", T=T_LONG, seed=31):
    maps, A, P, E, _ = CASES[case]
    grids = [grid(m) for m in maps]
    env_map = [e % len(grids) for e in range(E)]
    env = _mg().BatchedEnv(grids, E, A, P, T, seed=seed, env_map=env_map, tracker=tracker, shaping="qmix")
    env.reset()
    return env, [grids[m] for m in env_map]


def _ref(env, grids, cover=None):
    st = {k: v.cpu().numpy() for k, v in env.read_state().items() if k in ("robots", "pkgs")}
    return R.masks(grids, st["robots"], st["pkgs"], cover), st


def _random_mix(rs, codes, ref, p):
    """Each robot's action code replaced with probability p: half of those uniform over the 15
    actions, half uniform over the actions the rule leaves available."""
    E, A = codes.shape
    u = rs.rand(E, A)
    a = rs.randint(0, R.N_ACT, (E, A))
    for e, i in zip(*np.nonzero((u >= p / 2) & (u < p))):
        av = np.nonzero(ref[e, i])[0]
        a[e, i] = av[rs.randint(0, len(av))]
    rnd = (TRAINER_MOVE_CODES[a % 5] | ((a // 5) << 3)).astype(np.uint8)
    return np.where(u < p, rnd, codes)


@functools.lru_cache(maxsize=None)
def run_case(case, tracker):
    """The comparison along one rollout (the device's greedy agent, 40 % of the robots' actions
    replaced at random); returns what the rollout met: the rule's counters, pick-ups, deliveries."""
    env, grids = _make(case, tracker)
    cover, picks, drops = R.new_cover(), 0, 0
    if tracker != "fresh":
        env.clear_tracker()
    env.greedy_init()
    rs = np.random.RandomState(17)
    out = torch.empty((env.E, env.A, 15), dtype=torch.uint8, device=env.device)
    prev = None
    for k in range(CASES[case][4]):
        out.fill_(7)
        got = env.avail_actions(out=out)
        assert got is out
        ref, st = _ref(env, grids, cover)
        np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"{case} step {k}")
        if prev is not None:
            picks += int(((prev[..., 2] == 0) & (st["robots"][..., 2] != 0)).sum())
            drops += int(((prev[..., 2] != 0) & (st["robots"][..., 2] == 0)).sum())
        prev = st["robots"]
        codes = _random_mix(rs, env.greedy_actions().cpu().numpy(), ref, 0.4)
        env.step(torch.from_numpy(codes).to(env.device), auto_reset=False, action_format="codes")
    env.close()
    return cover, picks, drops


@pytest.mark.parametrize("case,tracker", RUNS)
def test_avail_actions_equals_the_rule_along_a_rollout(case, tracker):
    run_case(case, tracker)


def test_avail_actions_across_an_auto_reset():
    env, grids = _make("walls", T=10)
    rs = np.random.RandomState(3)
    resets = 0
    for k in range(30):
        ref, st = _ref(env, grids)
        np.testing.assert_array_equal(env.avail_actions().cpu().numpy(), ref, err_msg=f"step {k}")
        codes = _random_mix(rs, np.zeros((env.E, env.A), np.uint8), ref, 1.0)
        _, _, done = env.step(torch.from_numpy(codes).to(env.device), auto_reset=True, action_format="codes")
        resets += int(done.sum())
    assert resets >= 2 * env.E
    env.close()


def test_coverage_over_the_union_of_cases():
    """What the rollouts above met, summed (each runs once per session: ``run_case`` is cached)."""
    cover, picks, drops = R.new_cover(), 0, 0
    for case, tracker in RUNS:
        c, p, d = run_case(case, tracker)
        picks, drops = picks + p, drops + d
        for k in cover:
            cover[k] += c[k]
    print(cover, picks, drops)
    for k in R.COVER:
        assert cover[k] > 0, (k, cover)
    assert picks >= 20 and drops >= 5, (picks, drops)


# ---- the active argument
def test_active_mask_rows_state_and_refusals():
    mg = _mg()
    env, grids = _make("blocks")
    env.greedy_init()
    for _ in range(6):
        env.step(env.greedy_actions(), auto_reset=False, action_format="codes")
    before = env.save_state().tobytes()
    full = env.avail_actions()
    ref, _ = _ref(env, grids)
    np.testing.assert_array_equal(full.cpu().numpy(), ref)
    assert (ref == 0).any(-1).all()                               # every robot has a masked action: ones differ
    active = torch.from_numpy((np.random.RandomState(1).rand(env.E) < 0.5).astype(np.uint8)).to(env.device)
    keep = active.clone()
    got = env.avail_actions(active)
    on = active.bool().cpu().numpy()
    assert on.any() and (~on).any()
    assert bool((got[~active.bool()] == 1).all())                  # all ones exactly where the byte is 0
    np.testing.assert_array_equal(got.cpu().numpy()[on], ref[on])  # computed rows unchanged by the mask
    assert torch.equal(active, keep)                               # read, never written
    assert torch.equal(env.avail_actions(torch.ones_like(active)), full)
    assert bool((env.avail_actions(torch.zeros_like(active)) == 1).all())
    assert env.save_state().tobytes() == before                    # touches no state
    E, A = env.E, env.A
    u8 = dict(dtype=torch.uint8, device=env.device)
    for bad in (torch.ones(E, A, 15, dtype=torch.int32, device=env.device), torch.ones(E, A, 15, dtype=torch.uint8),
                torch.ones(E, A, 14, **u8), torch.ones(E * A * 15, **u8), torch.ones(E, 15, A, **u8).transpose(1, 2)):
        with pytest.raises((TypeError, ValueError)):
            env.avail_actions(out=bad)
    for bad in (torch.ones(E, dtype=torch.bool, device=env.device), torch.ones(E, dtype=torch.uint8),
                torch.ones(E - 1, **u8), torch.ones(2 * E, **u8)[::2]):
        with pytest.raises((TypeError, ValueError)):
            env.avail_actions(bad)
    assert env.save_state().tobytes() == before
    env.close()
    assert mg.BatchedEnv.avail_actions.__doc__


# ---- the masked sampler
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy uint32 arrays (tests/test_gpu_rollout.py's restatement)."""
    c = [np.asarray(x, np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c[0].astype(np.uint32)


def _uniforms(N, seed, off):
    rows = np.arange(N, dtype=np.uint64)
    u = philox(off & 0xFFFFFFFF, off >> 32, rows & 0xFFFFFFFF, rows >> 32, seed & 0xFFFFFFFF, seed >> 32) >> 8
    return u.astype(np.float64) * 2.0 ** -24


def _random_masks(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(N, K, generator=g) < 0.5).to(torch.uint8)
    m[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 1     # each row keeps at least one action
    return m


def test_masked_sampler_all_ones_is_the_unmasked_sampler():
    from marl_gpu.actions import sample_actions
    N, K = 20_000, 15
    logits = (torch.randn(N, K, generator=torch.Generator().manual_seed(1)) * 2).cuda()
    logits[5] = float("-inf")                                          # the sampler's all -inf row: action 0, -inf
    ones = torch.ones(N, K, dtype=torch.uint8, device="cuda")
    for off in (0, 7, (1 << 40) + 3):
        a0, l0 = sample_actions(logits, 0x1234_5678_9ABC_DEF0, off)
        a1, l1 = sample_actions(logits, 0x1234_5678_9ABC_DEF0, off, avail=ones)
        assert torch.equal(a0, a1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)), off
        a2, l2 = sample_actions(logits, 0x1234_5678_9ABC_DEF0, off, avail=ones.view(N // 5, 5, K).bool())
        assert torch.equal(a0, a2) and torch.equal(l0.view(torch.int32), l2.view(torch.int32)), off


def test_masked_sampler_matches_restatement_and_masked_softmax():
    from marl_gpu.actions import sample_actions, sample_actions_dev
    N, K = 100_000, 15
    logits = torch.randn(N, K, generator=torch.Generator().manual_seed(4)) * 2
    mask = _random_masks(N, K, 5)
    seed, off = 0x0FED_CBA9_8765_4321, 11
    a, lp = sample_actions(logits.cuda(), seed, off, avail=mask.cuda())
    a, lp = a.cpu().numpy(), lp.cpu()
    assert mask.numpy()[np.arange(N), a].all()                         # no unavailable action is returned
    masked = logits.masked_fill(mask == 0, float("-inf"))
    ref_lp = torch.log_softmax(masked, dim=1).gather(1, torch.from_numpy(a.astype(np.int64))[:, None])[:, 0]
    assert torch.allclose(lp, ref_lp, atol=3e-6, rtol=0)
    # inverse CDF of the masked softmax on the restated Philox uniform (fp64), skipping rows within 1e-5 of a bin edge
    u = _uniforms(N, seed, off)
    x = masked.double().numpy()
    p = np.exp(x - x.max(1, keepdims=True))
    cdf = np.cumsum(p, 1) / p.sum(1, keepdims=True)
    ref = (u[:, None] >= cdf).sum(1)
    safe = np.abs(cdf - u[:, None]).min(1) > 1e-5
    assert safe.mean() > 0.99
    assert np.array_equal(a[safe], ref[safe])
    # the _dev form at the same offset
    base = torch.tensor([off - 4], dtype=torch.int64, device="cuda")
    out = (torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.float32, device="cuda"))
    sample_actions_dev(logits.cuda(), seed, base, 4, out, avail=mask.cuda())
    assert np.array_equal(out[0].cpu().numpy(), a) and torch.equal(out[1].cpu().view(torch.int32), lp.view(torch.int32))
    # a row with no available action gets 0
    none = torch.zeros(3, K, dtype=torch.uint8, device="cuda")
    a0, l0 = sample_actions(logits[:3].cuda(), seed, off, avail=none)
    assert a0.tolist() == [0, 0, 0] and bool(torch.isinf(l0).all()) and bool((l0 < 0).all())
    with pytest.raises(ValueError):
        sample_actions(logits[:3].cuda(), seed, off, avail=torch.ones(3, K - 1, dtype=torch.uint8, device="cuda"))


def test_masked_sampler_frequencies():
    from marl_gpu.actions import sample_actions
    N, K = 200_000, 15
    row = torch.tensor([[0.3, -1.0, 2.0, 0.0, 0.5, -3.0, 1.0, 0.2, -0.5, 0.7, 0.0, -2.0, 1.5, 0.1, -0.1]])
    m = torch.tensor([[1, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1]], dtype=torch.uint8)
    b, _ = sample_actions(row.repeat(N, 1).cuda(), 99, 0, avail=m.repeat(N, 1).cuda())
    cnt = np.bincount(b.cpu().numpy(), minlength=K)
    keep = m[0].bool().numpy()
    assert cnt[~keep].sum() == 0
    exp = torch.softmax(row.double().masked_fill(m == 0, float("-inf")), 1)[0].numpy() * N
    chi2 = ((cnt[keep] - exp[keep]) ** 2 / exp[keep]).sum()
    assert chi2 < 45.0  # the unmasked test's statistic and threshold (there 14 dof; here 8)


# ---- the loops
HD = 16
COLLECT = dict(mapname="map1.txt", A=3, P=12, T=24, E=10, eps=0.5, env_seed=200, seed=11)
BATCH_KEYS = ("so", "vo", "gs", "gv", "u", "r", "r64", "r_shaped", "terminated", "filled", "hidden", "episode_return",
              "episode_length")


def make_agent(dv):
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
    g = torch.Generator().manual_seed(35)
    with torch.no_grad():
        for p in a.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    return a.cuda()


def make_env(tracker="fresh"):
    c = COLLECT
    return _mg().BatchedEnv(grid(c["mapname"]), c["E"], c["A"], c["P"], c["T"], seed=c["env_seed"], tracker=tracker,
                            shaping="qmix")


def snapshot(batch, keys=BATCH_KEYS + ("avail",)):
    return {k: batch[k].clone() for k in keys}


def assert_same(x, y, what):
    assert x.keys() == y.keys()
    for k in x:
        assert torch.equal(x[k].view(torch.uint8) if x[k].is_floating_point() else x[k],
                           y[k].view(torch.uint8) if y[k].is_floating_point() else y[k]), f"{what}: {k}"


def test_collector_with_avail_equals_hand_written_loop():
    import marl_gpu.qmix_rollout as Q
    c = COLLECT
    E, A, L = c["E"], c["A"], c["T"]
    env = make_env()
    agent = make_agent(env.actor_vec_dim)
    col = Q.QmixCollector(env, episode_limit=100, seed=c["seed"], avail=True)
    b = col.collect(agent, c["eps"])
    assert b["avail"].shape == (L + 1, E, A, 15) and b["avail"].dtype == torch.uint8

    ref = make_env()
    hand = Q.QmixCollector(ref, episode_limit=100, seed=c["seed"])     # only its (zeroed) buffers are used
    masks = torch.zeros((L + 1, E, A, 15), dtype=torch.uint8, device="cuda")
    ref.reset()
    active = torch.ones(E, dtype=torch.uint8, device="cuda")
    ref.build_obs(out=hand._slot(0))
    ref.avail_actions(active, out=masks[0])
    h = agent.init_hidden().expand(E * A, -1)
    agent.eval()
    unmasked_differs = 0
    with torch.no_grad():
        for t in range(L):
            q, h = agent(hand.so[t].reshape(E * A, *hand.so.shape[3:]), hand.vo[t].reshape(E * A, -1), h)
            Q.select_actions_eps(q, c["eps"], c["seed"], t, avail=masks[t], out=hand.u[t].view(-1))
            unmasked_differs += int((Q.select_actions_eps(q, c["eps"], c["seed"], t) != hand.u[t].view(-1)).sum())
            ref.step_episode(hand.u[t], active, out=(hand.r64[t], hand.r_shaped[t], hand.terminated[t]),
                             filled=hand.filled[t], obs_out=hand._slot(t + 1))
            ref.avail_actions(active, out=masks[t + 1])
    for k in ("so", "vo", "gs", "gv", "u", "r64", "r_shaped", "terminated", "filled"):
        assert torch.equal(b[k], getattr(hand, k)), k
    assert torch.equal(b["avail"], masks)
    assert env.save_state().tobytes() == ref.save_state().tobytes()
    # every action of a running env was available; the masks mask something; a finished env's rows are ones
    took = torch.gather(b["avail"][:L], 3, b["u"].long().unsqueeze(-1))[..., 0]
    assert bool((took == 1).all())
    assert bool((b["avail"] == 0).any())
    over = ~torch.cat((torch.ones(1, E, dtype=torch.bool, device="cuda"), b["filled"].bool() & ~b["terminated"].bool()))
    assert bool(over.any()) and bool((b["avail"][over] == 1).all())
    assert unmasked_differs > 0     # the mask changes what is selected: the same q and draws, unmasked
    env.close()
    ref.close()


def test_collector_avail_graph_replay_equals_eager():
    import marl_gpu.qmix_rollout as Q
    c = COLLECT
    env_e, env_g = make_env(), make_env()
    agent = make_agent(env_e.actor_vec_dim)
    eager = Q.QmixCollector(env_e, c["T"], seed=c["seed"], avail=True)
    graph = Q.QmixCollector(env_g, c["T"], seed=c["seed"], avail=True)
    for call, (eps, use_graph) in enumerate(((c["eps"], True), (0.35, True), (0.6, False), (0.2, True))):
        x = snapshot(eager.collect(agent, eps))                        # capture, replay, eager, replay
        y = snapshot(graph.collect(agent, eps, graph=use_graph))
        assert_same(x, y, f"call {call}")
        assert env_e.save_state().tobytes() == env_g.save_state().tobytes()
        assert eager.offset == graph.offset == (call + 1) * c["T"]
    assert graph.captured_graphs() == {None: c["T"]}
    env_e.close()
    env_g.close()


def test_collector_avail_off_is_the_collector_without_the_argument():
    import marl_gpu.qmix_rollout as Q
    c = COLLECT
    env_a, env_b = make_env(), make_env()
    agent = make_agent(env_a.actor_vec_dim)
    a = Q.QmixCollector(env_a, c["T"], seed=c["seed"], avail=False)
    b = Q.QmixCollector(env_b, c["T"], seed=c["seed"])
    for graph in (False, True, True):
        x, y = a.collect(agent, c["eps"], graph=graph), b.collect(agent, c["eps"], graph=graph)
        assert "avail" not in x and "avail" not in y
        assert_same(snapshot(x, BATCH_KEYS), snapshot(y, BATCH_KEYS), f"graph={graph}")
    env_a.close()
    env_b.close()


def test_episode_replay_round_trip_on_the_device():
    import marl_gpu.qmix_rollout as Q
    c = COLLECT
    L = c["T"]
    env = make_env()
    agent = make_agent(env.actor_vec_dim)
    col = Q.QmixCollector(env, L, seed=c["seed"], avail=True)
    rp = Q.EpisodeReplay(2 * c["E"], col)
    first = snapshot(col.collect(agent, c["eps"]))
    rp.add(first)
    second = snapshot(col.collect(agent, c["eps"]))
    rp.add(second)
    stored = torch.cat((first["avail"], second["avail"]), 1)
    assert torch.equal(rp.buf["avail"], stored)
    s = rp.sample(7, generator=torch.Generator().manual_seed(3))
    idx = torch.randperm(2 * c["E"], generator=torch.Generator().manual_seed(3))[:7].cuda()
    want = stored[:, idx].transpose(0, 1).float()
    assert torch.equal(s["avail_u"], want[:, :L]) and torch.equal(s["avail_u_next"], want[:, 1:])
    assert s["avail_u"].is_cuda and s["avail_u"].shape == (7, L, c["A"], 15)
    u = torch.cat((first["u"], second["u"]), 1)[:, idx].transpose(0, 1).long().unsqueeze(-1)
    assert torch.equal(s["u"], u)
    assert bool((torch.gather(s["avail_u"], 3, s["u"]) == 1).all())    # the stored action under the stored mask
    plain = Q.EpisodeReplay(4, Q.QmixCollector(env, L, seed=c["seed"]))
    assert "avail" not in plain.buf
    env.close()


class _LinearActor(torch.nn.Module):
    def __init__(self, H, W, Dv, device):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.wm = torch.nn.Parameter((torch.randn(6 * H * W, 15, generator=g) * 0.3).to(device))
        self.wv = torch.nn.Parameter(torch.randn(Dv, 15, generator=g).to(device))

    def forward(self, amap, avec):
        return amap.reshape(amap.shape[0], -1) @ self.wm + avec @ self.wv


class _Spy:
    """A policy that also records, at every call, the evaluator's action buffer (the actions of the
    step before) and the mask of the state it is asked about.  For eager runs."""

    def __init__(self, policy, ev):
        self.policy, self.ev, self.acts, self.masks, self.active = policy, ev, [], [], []

    def __call__(self, amap, avec):
        self.acts.append(self.ev.actions.clone())
        self.active.append(self.ev.active.clone())
        self.masks.append(self.ev.env.avail_actions(self.ev.active))
        return self.policy(amap, avec)

    def taken(self):
        """(masks [L, E, A, 15], actions [L, E, A], active [L, E]): step k's, for every step of the run."""
        acts = self.acts[1:] + [self.ev.actions.clone()]
        return torch.stack(self.masks), torch.stack(acts), torch.stack(self.active)


@pytest.mark.parametrize("deterministic", [True, False])
def test_evaluator_with_avail(deterministic):
    mg = _mg()
    E, A, P, T = 12, 3, 8, 20

    def make():
        return mg.BatchedEnv(grid("map1.txt"), E, A, P, T, seed=70, tracker="fresh")

    env, env_p, env_o, env_g = make(), make(), make(), make()
    H, W = env.single_map_shape("test")
    policy = _LinearActor(H, W, env.actor_vec_dim, env.device)
    ev = mg.Evaluator(env, seed=5)
    spy = _Spy(policy, ev)
    masked = {k: v.clone() for k, v in ev.run(spy, deterministic=deterministic, avail=True).items()}
    state = env.save_state().tobytes()
    m, a, on = spy.taken()
    took = torch.gather(m, 3, a.long().unsqueeze(-1))[..., 0]
    assert bool((took[on.bool()] == 1).all())                          # every chosen action is available
    # without the mask the same policy takes unavailable actions (the check above is not vacuous)
    ev_p = mg.Evaluator(env_p, seed=5)
    spy = _Spy(policy, ev_p)
    plain = {k: v.clone() for k, v in ev_p.run(spy, deterministic=deterministic).items()}
    m, a, on = spy.taken()
    assert bool((torch.gather(m, 3, a.long().unsqueeze(-1))[..., 0][on.bool()] == 0).any())
    # off == a run without the argument
    for k, v in mg.Evaluator(env_o, seed=5).run(policy, deterministic=deterministic, avail=False).items():
        assert torch.equal(v, plain[k]), k
    assert env_o.save_state().tobytes() == env_p.save_state().tobytes()
    # graph == eager: the capturing call and a replay, against the first and a second eager run
    second = {k: v.clone() for k, v in ev.run(policy, deterministic=deterministic, avail=True).items()}
    ev_g = mg.Evaluator(env_g, seed=5)
    for want, st in ((masked, state), (second, env.save_state().tobytes())):
        for k, v in ev_g.run(policy, deterministic=deterministic, graph=True, graph_steps=8, avail=True).items():
            assert torch.equal(v, want[k]), k
        assert env_g.save_state().tobytes() == st
    assert set(ev_g.captured_graphs()) == {"chunk", "rest"} and ev.offset == ev_g.offset
    # avail is part of the graph key
    key = ("policy", T, 8, deterministic)
    assert ev_g._graphs.matches((policy,), key + (True,)) and not ev_g._graphs.matches((policy,), key + (False,))
    for e in (env, env_p, env_o, env_g):
        e.close()


def test_mappo_rollout_with_avail():
    mg = _mg()
    from marl_gpu.rollout import MappoRollout
    g = grid("map1.txt")
    E, A, P, T, steps = 12, 5, 30, 14, 10        # T < 2 * steps: auto-resets inside the rollouts

    def make():
        env = mg.BatchedEnv(g, E, A, P, T, seed=7, tracker="mappo", shaping="mappo", max_other_robots=A - 1,
                            max_packages_obs=5)
        env.reset()
        return env

    gen = torch.Generator(device="cuda").manual_seed(3)
    envs = [make() for _ in range(4)]
    wa = torch.randn(envs[0].actor_vec_dim, 15, device="cuda", generator=gen)
    wc = torch.randn(envs[0].critic_vec_dim, device="cuda", generator=gen) * 0.01

    def actor(obs, vec):
        return vec @ wa * 0.1 + obs.sum(dim=(1, 2, 3)).unsqueeze(1) * 0.01

    def critic(gmap, gvec):
        return gvec @ wc

    eager, graphed = MappoRollout(envs[0], steps, seed=5, avail=True), MappoRollout(envs[1], steps, seed=5, avail=True)
    off, plain = MappoRollout(envs[2], steps, seed=5, avail=False), MappoRollout(envs[3], steps, seed=5)
    first = envs[0].avail_actions().clone()
    for call in range(3):   # call 0 captures; calls 1, 2 replay
        a = [x.clone() for x in eager.collect(actor, critic)]
        b = [x.clone() for x in graphed.collect(actor, critic, graph=True)]
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"rollout {call}, output {i}"
        assert torch.equal(eager.mb_avail, graphed.mb_avail)
        if call == 0:
            assert torch.equal(eager.mb_avail[0], first)
        took = torch.gather(eager.mb_avail, 3, eager.mb_actions.long().unsqueeze(-1))[..., 0]
        assert bool((took == 1).all()) and bool((eager.mb_avail == 0).any())
        assert bool(torch.isfinite(eager.mb_log_probs).all())
        c = [x.clone() for x in off.collect(actor, critic)]
        d = [x.clone() for x in plain.collect(actor, critic)]
        for i, (x, y) in enumerate(zip(c, d)):
            assert torch.equal(x, y), f"rollout {call}, output {i} (avail off)"
        # the unmasked rollout does take actions its own states mask
        assert not torch.equal(a[4], c[4])
    assert envs[0].save_state().tobytes() == envs[1].save_state().tobytes()
    assert envs[2].save_state().tobytes() == envs[3].save_state().tobytes()
    assert off.mb_avail is None and plain.mb_avail is None
    assert eager.offset == graphed.offset == 3 * steps
    for e in envs:
        e.close()
