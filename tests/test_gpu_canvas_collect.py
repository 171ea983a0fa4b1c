"""MappoRollout(canvas=) and QmixCollector(canvas=): on one map shape against a twin without a canvas (every
tensor and the engine state equal, eager and graphed); on an engine that mixes three map shapes against the
CPU oracle replaying the collector's own actions, slot by slot and bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import canvas_ref as V  # noqa: E402
import ego_ref as G  # noqa: E402
import oracle as O  # noqa: E402
from ego_masked_ref import SENTINEL_BITS  # noqa: E402
from golden_io import grid  # noqa: E402
from test_gpu_canvas import bits, make_env, same, sentinel, want_bits  # noqa: E402

F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


def policies(env, seed=3):
    """A small fixed-seed actor and critic that read every input: the window's and the canvas's channels
    weigh in, so a wrong map tensor changes the actions and the values."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    wa = torch.randn(env.actor_vec_dim, 15, device="cuda", generator=gen)
    wm = torch.randn(6, 15, device="cuda", generator=gen) * 0.05
    wc = torch.randn(env.critic_vec_dim, device="cuda", generator=gen) * 0.01
    wg = torch.randn(4, device="cuda", generator=gen) * 0.01

    def actor(obs, vec):
        return vec @ wa + obs.sum(dim=(2, 3)) @ wm

    def critic(gmap, gvec):
        return gvec @ wc + gmap.mean(dim=(2, 3)) @ wg

    return actor, critic


class Agent:
    """A recurrent Q-network stand-in with the reference's interface (init_hidden, forward -> q, h')."""

    def __init__(self, env, hd=8, seed=5):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.wv = torch.randn(env.actor_vec_dim, hd, device="cuda", generator=gen) * 0.3
        self.wm = torch.randn(6, hd, device="cuda", generator=gen) * 0.05
        self.wh = torch.randn(hd, hd, device="cuda", generator=gen) * 0.3
        self.wq = torch.randn(hd, 15, device="cuda", generator=gen)
        self.hd = hd

    def init_hidden(self):
        return torch.zeros(1, self.hd, device="cuda")

    def __call__(self, so, vo, h):
        h = torch.tanh(vo @ self.wv + so.float().sum(dim=(2, 3)) @ self.wm + h @ self.wh)
        return h @ self.wq, h


class Scripted:
    """An agent that plays recorded trainer ints [T, E, A] whatever it sees: its hidden state counts the
    steps (on the device, so a captured collect replays it), its Q-values are one-hot at the recorded action."""

    def __init__(self, ints):
        T, E, A = ints.shape
        hot = np.zeros((T + 1, E * A, 15), np.float32)
        hot[np.arange(T)[:, None], np.arange(E * A)[None, :], ints.reshape(T, E * A)] = 1
        self.table = torch.from_numpy(hot).cuda()
        self.T = T

    def init_hidden(self):
        return torch.zeros(1, 1, device="cuda")

    def __call__(self, so, vo, h):
        q = self.table.index_select(0, h[0, :1].long().clamp(max=self.T))[0]
        return q, h + 1


def test_canvas_needs_a_radius():
    import marl_gpu
    from marl_gpu.qmix_rollout import QmixCollector
    from marl_gpu.rollout import MappoRollout
    env = marl_gpu.BatchedEnv(grid("map1.txt"), 4, 3, 8, 10, seed=1)
    mixed = make_env(V.BY_ID["mixed_fresh"])
    try:
        with pytest.raises(ValueError, match="ego_radius"):
            MappoRollout(env, 4, canvas=(10, 10))
        with pytest.raises(ValueError, match="ego_radius"):
            QmixCollector(env, 4, canvas=(10, 10))
        with pytest.raises(ValueError):
            MappoRollout(env, 4, ego_radius=2, canvas=(10, 256))
        # canvas=None keeps the refusal of a mixed engine
        with pytest.raises(ValueError, match="mix map shapes"):
            MappoRollout(mixed, 4, ego_radius=2)
        with pytest.raises(ValueError, match="mix map shapes"):
            QmixCollector(mixed, 4, ego_radius=2)
        assert tuple(MappoRollout(mixed, 4, ego_radius=2, canvas=(20, 21)).mb_global_states.shape) == (4, 8, 4, 20, 21)
        assert tuple(QmixCollector(mixed, 4, ego_radius=2, canvas=(20, 21)).gs.shape) == (5, 8, 4, 20, 21)
    finally:
        env.close()
        mixed.close()


def test_mappo_twin_on_one_shape():
    """MappoRollout(ego_radius=2, canvas=(H, W)) against MappoRollout(ego_radius=2) on map1: every returned
    tensor, buffer and the engine state are equal, eager and graph=True, over two collects each."""
    import marl_gpu
    from marl_gpu.rollout import MappoRollout
    g = grid("map1.txt")
    E, A, P, T, steps = 8, 5, 20, 10, 6

    def make():
        env = marl_gpu.BatchedEnv(g, E, A, P, T, seed=7, tracker="mappo", shaping="mappo", max_packages_obs=5)
        env.reset()
        return env

    envs = [make() for _ in range(3)]
    actor, critic = policies(envs[0])
    try:
        twin = MappoRollout(envs[0], steps, seed=5, ego_radius=2)
        eager = MappoRollout(envs[1], steps, seed=5, ego_radius=2, canvas=(10, 10))
        graphed = MappoRollout(envs[2], steps, seed=5, ego_radius=2, canvas=(10, 10))
        for k in range(2):   # call 0 of `graphed` runs eagerly and captures, call 1 replays
            a = [x.clone() for x in twin.collect(actor, critic)]
            b = [x.clone() for x in eager.collect(actor, critic)]
            c = [x.clone() for x in graphed.collect(actor, critic, graph=True)]
            torch.cuda.synchronize()
            for i, (x, y, z) in enumerate(zip(a, b, c)):
                assert torch.equal(x, y), f"collect {k}, output {i}: eager"
                assert torch.equal(x, z), f"collect {k}, output {i}: graphed"
            for name in ("mb_obs", "mb_vector_obs", "mb_global_states", "mb_global_vector", "mb_actions",
                         "mb_log_probs", "mb_rewards", "mb_dones", "mb_values"):
                for other in (eager, graphed):
                    assert torch.equal(getattr(twin, name), getattr(other, name)), f"collect {k}: {name}"
            for key in twin.next_obs:
                for other in (eager, graphed):
                    assert torch.equal(twin.next_obs[key], other.next_obs[key]), f"collect {k}: next_obs[{key}]"
        assert graphed.captured_graphs() == {None: steps}
        s0, s1, s2 = (e.save_state() for e in envs)
        assert np.array_equal(s0, s1) and np.array_equal(s0, s2)
    finally:
        for e in envs:
            e.close()


def test_qmix_twin_on_one_shape():
    """QmixCollector(ego_radius=2, canvas=(H, W)) against QmixCollector(ego_radius=2): rows past an episode's
    end are pre-filled with a sentinel on both sides, so the unwritten rows must agree too."""
    import marl_gpu
    from marl_gpu.qmix_rollout import QmixCollector
    import ego_masked_ref as M
    ep = M.EPISODE   # greedy episodes on map1 that end at different steps (test_ego_masked_cpu.py)
    g = grid(ep.map)
    E, A, P, T = ep.E, ep.A, ep.P, ep.T

    def make():
        return marl_gpu.BatchedEnv(g, E, A, P, T, seed=ep.seed, tracker="fresh", shaping="qmix", max_packages_obs=5)

    envs = [make() for _ in range(3)]
    tr = M.episode_trace(ep)
    agent = Scripted(tr["ints"])   # the oracle's greedy actions of the first episode
    try:
        cols = [QmixCollector(envs[0], T, seed=9, ego_radius=2),
                QmixCollector(envs[1], T, seed=9, ego_radius=2, canvas=(10, 10)),
                QmixCollector(envs[2], T, seed=9, ego_radius=2, canvas=(10, 10))]
        for k in range(2):
            for c in cols:
                for name in ("so", "vo", "gs", "gv"):
                    t = getattr(c, name)
                    t.copy_(sentinel(t.shape, t.dtype))
            outs = [c.collect(agent, 0.0, graph=(i == 2)) for i, c in enumerate(cols)]
            torch.cuda.synchronize()
            for key in outs[0]:
                for i in (1, 2):
                    assert bits_equal(outs[0][key], outs[i][key]), f"collect {k}: {key} of collector {i}"
            L = outs[0]["episode_length"].cpu().numpy()
            if k == 0:
                assert L.tolist() == tr["length"].tolist() and (L < T).any(), L   # episodes end at different steps
                assert (bits(outs[1]["gs"][T]) == SENTINEL_BITS[4]).any()         # rows past an end stay unwritten
        assert np.array_equal(envs[0].save_state(), envs[1].save_state())
        assert np.array_equal(envs[0].save_state(), envs[2].save_state())
    finally:
        for e in envs:
            e.close()


def bits_equal(a, b):
    if a.dtype in (torch.float32, torch.float16, torch.bfloat16):
        return bits(a).tobytes() == bits(b).tobytes()   # the sentinel is a NaN: compare bits
    return torch.equal(a, b)


def test_mappo_on_mixed_maps_against_the_oracle():
    """mixed_stale: T_rollout = 12 with T = 10, so every env auto-resets once.  The oracle replays mb_actions;
    every slot of every observation buffer, the rewards and the dones are its own."""
    from marl_gpu.rollout import MappoRollout
    case = V.BY_ID["mixed_stale"]
    canvas, R, steps = (21, 23), 2, 12
    E, A = case.E, case.A
    envs = [make_env(case) for _ in range(2)]
    actor, critic = policies(envs[0])
    try:
        for e in envs:
            e.reset()
        ro = MappoRollout(envs[0], steps, seed=5, ego_radius=R, canvas=canvas)
        gr = MappoRollout(envs[1], steps, seed=5, ego_radius=R, canvas=canvas)
        assert tuple(ro.mb_global_states.shape) == (steps, E, 4) + canvas
        assert tuple(ro.next_obs["critic_map"].shape) == (E, 4) + canvas
        first = [x.clone() for x in ro.collect(actor, critic)]
        torch.cuda.synchronize()
        ref = V.Replay(V.base(case))
        acts = ro.mb_actions.cpu().numpy()
        resets = 0

        def check(slot, what):
            obs = ref.obs_all()
            want = V.want(obs, canvas)
            ego = np.stack([G.ego_from_full(o["actor_map"], R) for o in obs])
            same(bits(slot["actor_map"]), want_bits(ego, F32), f"{what}: windows")
            same(bits(slot["actor_vec"]), want_bits(want["actor_vec"], F32), f"{what}: actor_vec")
            same(bits(slot["critic_map"]), want_bits(want["critic_map"], F32), f"{what}: canvas")
            same(bits(slot["critic_vec"]), want_bits(want["critic_vec"], F32), f"{what}: critic_vec")

        for k in range(steps):
            check(ro._slot(k), f"slot {k}")
            _, sh, dn = ref.step(acts[k])
            same(bits(ro.mb_rewards[k]), sh.view(np.uint32), f"step {k}: rewards")
            assert np.array_equal(ro.mb_dones[k].cpu().numpy().astype(bool), dn), f"step {k}: dones"
            resets += int(dn.sum())
        check(ro.next_obs, "next_obs")
        assert resets == E
        assert torch.equal(first[2], ro.mb_global_states.reshape(steps * E, 4, *canvas))
        # a second collect through the graph equals an eager twin's second collect
        gr.collect(actor, critic, graph=True)
        a = [x.clone() for x in ro.collect(actor, critic)]
        b = [x.clone() for x in gr.collect(actor, critic, graph=True)]
        torch.cuda.synchronize()
        assert gr.captured_graphs() == {None: steps}
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"second collect, output {i}"
        for key in ro.next_obs:
            assert torch.equal(ro.next_obs[key], gr.next_obs[key]), key
        assert np.array_equal(envs[0].save_state(), envs[1].save_state())
    finally:
        for e in envs:
            e.close()


def test_qmix_on_mixed_maps_against_the_oracle():
    """mixed_fresh with QmixCollector(ego_radius=3, canvas=(21, 23), episode_limit=10): the oracle replays u
    without resets.  Written rows (slot 0, and slot t + 1 where filled[t]) are the oracle's, unwritten rows
    keep the sentinel; the terminal observation of an env that finishes at step t is written (filled[t] is
    set, active is already cleared); returns and lengths are the oracle's; EpisodeReplay keeps the shape."""
    from marl_gpu.qmix_rollout import QmixCollector
    from marl_gpu.replay import EpisodeReplay
    case = V.BY_ID["mixed_fresh"]
    canvas, R, L = (21, 23), 3, 10
    E, A = case.E, case.A
    envs = [make_env(case, shaping="qmix") for _ in range(2)]
    agent = Agent(envs[0])
    try:
        cols = [QmixCollector(e, L, seed=9, ego_radius=R, canvas=canvas) for e in envs]
        col = cols[0]
        assert tuple(col.gs.shape) == (L + 1, E, 4) + canvas
        for c in cols:
            for name in ("so", "vo", "gs", "gv"):
                t = getattr(c, name)
                t.copy_(sentinel(t.shape, t.dtype))
        b = col.collect(agent, 0.25)
        g = cols[1].collect(agent, 0.25, graph=True)
        torch.cuda.synchronize()
        ref = V.Replay(V.base(case), consts=O.QMIX_CONSTS, auto_reset=False)
        u = b["u"].cpu().numpy()
        filled = b["filled"].cpu().numpy().astype(bool)
        running = np.ones(E, bool)
        got = {k: bits(b[k]) for k in ("so", "vo", "gs", "gv")}

        def check(t, rows, what):
            obs = ref.obs_all()
            want = V.want(obs, canvas)
            ego = np.stack([G.ego_from_full(o["actor_map"], R) for o in obs])
            exp = dict(so=want_bits(ego, F32), vo=want_bits(want["actor_vec"], F32),
                       gs=want_bits(want["critic_map"], F32), gv=want_bits(want["critic_vec"], F32))
            for k, x in exp.items():
                x = x.copy()
                x[~rows] = SENTINEL_BITS[4]
                same(got[k][t], x, f"{what}: {k}")

        check(0, running, "slot 0")
        terminal = 0
        for t in range(L):
            assert np.array_equal(filled[t], running), f"step {t}: filled"
            r, sh, dn = ref.step(u[t], running)
            assert b["r64"][t].cpu().numpy().tobytes() == r.tobytes(), f"step {t}: r64"
            same(bits(b["r_shaped"][t]), sh.view(np.uint32), f"step {t}: r_shaped")
            assert np.array_equal(b["terminated"][t].cpu().numpy().astype(bool), dn), f"step {t}: terminated"
            check(t + 1, running, f"slot {t + 1}")   # the envs that just finished included
            terminal += int(dn.sum())
            running = running & ~dn
        assert terminal == E and not running.any()
        assert not col.active.any()
        want_ret = np.array([ref.total_reward(e) for e in range(E)], np.float64)
        assert b["episode_return"].cpu().numpy().tobytes() == want_ret.tobytes()
        assert np.array_equal(b["episode_length"].cpu().numpy(), filled.sum(0))
        # the graphed collector's first call ran eagerly: the same episodes; its replay matches an eager twin
        for k in b:
            assert bits_equal(b[k], g[k]), f"first collect: {k}"
        b = col.collect(agent, 0.25)
        g = cols[1].collect(agent, 0.25, graph=True)
        torch.cuda.synchronize()
        assert cols[1].captured_graphs() == {None: L}
        for k in b:
            assert bits_equal(b[k], g[k]), f"second collect: {k}"
        # EpisodeReplay takes its shapes from the collector's tensors
        rep = EpisodeReplay(E, col)
        assert tuple(rep.buf["gs"].shape) == (L + 1, E, 4) + canvas
        rep.add(b)
        assert bits_equal(rep.buf["gs"], b["gs"]) and bits_equal(rep.buf["so"], b["so"])
        s = rep.sample(E, generator=torch.Generator(device="cuda").manual_seed(1))
        assert tuple(s["gs"].shape) == (E, L, 4) + canvas and tuple(s["gs_next"].shape) == (E, L, 4) + canvas
        assert tuple(s["so"].shape) == (E, L, A, 6, 2 * R + 1, 2 * R + 1)
        pool = [bits(b["gs"][:, e]).tobytes() for e in range(E)]
        for i in range(E):   # every sampled episode is one of the stored ones, slots 0..L-1 and 1..L
            whole = bits(torch.cat([s["gs"][i], s["gs_next"][i, -1:]])).tobytes()
            assert whole in pool, i
    finally:
        for e in envs:
            e.close()
