"""IdqCollector(ego_radius=) and QmixCycleCollector(ego_radius=) against full-map twins, on
ego_masked_ref.EPISODE's shape.  The agents' q is a one-hot of the device's greedy action and never reads
the observations, so a window-form collector and its twin act alike and the deliveries end episodes at
different steps: everything but the observations is equal, and the observations are
alt_ego_ref.alt_ego_from_full of the twin's, bit for bit.  graph=True equals eager; a replay of the wrong
obs_shape is refused; ego_radius=None is the default path."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import alt_ego_ref as X  # noqa: E402
import ego_masked_ref as M  # noqa: E402
import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402

EP = M.EPISODE
R, K = EP.R, 2 * EP.R + 1
HW = (10, 10)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()
    assert grid(EP.map).shape == HW and R == 2


def episode_env():
    import marl_gpu
    return marl_gpu.BatchedEnv(grid(EP.map), EP.E, EP.A, EP.P, EP.T, seed=EP.seed, tracker="fresh", shaping="qmix")


def raw(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def crop(t):
    """alt_ego_from_full of a device tensor [.., 6, H, W] of whole rows, as bit patterns."""
    return np.ascontiguousarray(X.alt_ego_from_full(t.cpu().numpy(), R)).view(np.uint32)


class GreedyQ:
    """q = one-hot of the device's greedy action as a trainer int.  every: the agent is called that many
    times per episode batch and re-makes the greedy agents at the first (0: the caller does)."""

    def __init__(self, env, every=0):
        self.env, self.every, self.calls, self.col, self.seen = env, every, 0, None, []
        self.lut = torch.from_numpy(M.INT_OF_CODE.astype(np.int64)).cuda()

    def __call__(self, obs):
        if self.every and self.calls % self.every == 0:
            self.env.greedy_init()
        self.calls += 1
        self.seen.append(tuple(obs.shape))
        codes = self.env.greedy_actions_masked(self.col.active if self.every else None)
        q = torch.zeros((codes.numel(), 15), dtype=torch.float32, device="cuda")
        return q.scatter_(1, self.lut[codes.view(-1).long()].unsqueeze(1), 1.0)


def close_all(made):
    for m in made:
        m[0].close()


# ---------------------------------------------------------------- IdqCollector
def make_idq(capacity, **kw):
    from marl_gpu.idq_rollout import IdqCollector
    from marl_gpu.replay import TransitionReplay
    env = episode_env()
    shape = (6, K, K) if kw.get("ego_radius") else (6,) + HW
    rep = TransitionReplay(capacity, shape, device="cuda")
    col = IdqCollector(env, rep, seed=3, ops_are_ints=True, **kw)
    ag = GreedyQ(env, every=EP.T)
    ag.col = col
    return env, ag, col, rep


IDQ_SAME = ("u", "r_idq", "r_env", "filled", "done", "episode_return")
RING_SAME = ("actions", "rewards", "dones")


def test_idq_collector_with_windows_against_a_full_map_twin():
    made = [make_idq(1100), make_idq(1100, ego_radius=R)]
    try:
        (_, ag_f, full, rep_f), (_, ag_e, ego, rep_e) = made
        assert tuple(ego.obs.shape) == (2, EP.E, EP.A, 6, K, K) and tuple(full.obs.shape) == (2, EP.E, EP.A, 6) + HW
        rows = 0
        for call in range(2):   # the second collect plays the next layouts of the same streams
            full.collect(ag_f, 0.0)
            ego.collect(ag_e, 0.0)
            torch.cuda.synchronize()
            for k in IDQ_SAME:
                assert torch.equal(getattr(full, k), getattr(ego, k)), f"collect {call}: {k}"
            assert torch.equal(rep_f.cursor, rep_e.cursor), f"collect {call}: the ring cursor"
            ptr_, size = rep_e.position()
            assert ptr_ == size and size > rows   # no wrap: rows [0, size) are the filled rows, in order
            if call == 0:   # ego_masked_ref's episodes: they end at different steps
                assert size == EP.A * int(M.episode_trace(EP)["length"].sum()) < EP.A * EP.E * EP.T
            rows = size
            for k in RING_SAME:
                assert torch.equal(getattr(rep_f, k)[:size], getattr(rep_e, k)[:size]), f"collect {call}: ring {k}"
            for k in ("observations", "next_observations"):
                assert raw(getattr(rep_e, k)[:size]).tobytes() == crop(getattr(rep_f, k)[:size]).tobytes(), \
                    f"collect {call}: ring {k} are not the crops of the twin's"
            assert not raw(getattr(rep_e, "observations")[size:]).any()
        assert ag_e.seen[0] == (EP.E * EP.A, 6, K, K) and ag_f.seen[0] == (EP.E * EP.A, 6) + HW
        assert raw(rep_e.observations[:rows, 1]).any()   # urgencies reached the ring
    finally:
        close_all(made)


def test_idq_collector_with_windows_graph_equals_eager():
    made = [make_idq(600, ego_radius=R), make_idq(600, ego_radius=R)]
    try:
        (_, ag_a, eager, rep_a), (_, ag_b, graphed, rep_b) = made
        for call in range(3):   # call 0 of `graphed` runs eagerly and captures, calls 1 and 2 replay
            eager.collect(ag_a, 0.0)
            graphed.collect(ag_b, 0.0, graph=True)
            torch.cuda.synchronize()
            for k in IDQ_SAME:
                assert torch.equal(getattr(eager, k), getattr(graphed, k)), f"collect {call}: {k}"
            assert torch.equal(rep_a.cursor, rep_b.cursor)
            assert raw(eager.obs).tobytes() == raw(graphed.obs).tobytes(), f"collect {call}: obs"
            for k in RING_SAME + ("observations", "next_observations"):
                a, b = getattr(rep_a, k), getattr(rep_b, k)
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"collect {call}: ring {k}"
        assert graphed.captured_graphs() == {None: EP.T}
        assert rep_b.position()[1] == 600   # the ring wrapped: both wrapped alike
    finally:
        close_all(made)


def test_idq_collector_default_is_the_full_map_path():
    made = [make_idq(600), make_idq(600, ego_radius=None)]
    try:
        (_, ag_a, a, rep_a), (_, ag_b, b, rep_b) = made
        assert a.ego_radius is None and b.ego_radius is None
        a.collect(ag_a, 0.0)
        b.collect(ag_b, 0.0)
        torch.cuda.synchronize()
        for k in IDQ_SAME + ("obs",):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        for k in RING_SAME + ("observations", "next_observations", "cursor"):
            assert torch.equal(getattr(rep_a, k), getattr(rep_b, k)), k
    finally:
        close_all(made)


# ---------------------------------------------------------------- QmixCycleCollector
def make_cycle(capacity, **kw):
    from marl_gpu.qmix_cycle import QmixCycleCollector
    from marl_gpu.replay import JointReplay
    env = episode_env()
    shape = (6, K, K) if kw.get("ego_radius") else (6,) + HW
    rep = JointReplay(capacity, EP.A, shape, (7,) + HW, device="cuda")
    col = QmixCycleCollector(env, rep, seed=3, **kw)
    ag = GreedyQ(env)
    ag.col = col
    col.begin()
    env.greedy_init()
    return env, ag, col, rep


CYCLE_SAME = ("state", "u", "r_env", "done", "completed_steps")
JOINT_SAME = ("states", "next_states", "actions", "total_reward", "dones")


def test_cycle_collector_with_windows_against_a_full_map_twin():
    made = [make_cycle(200), make_cycle(200, ego_radius=R)]
    try:
        (_, ag_f, full, rep_f), (_, ag_e, ego, rep_e) = made
        assert tuple(ego.obs.shape) == (2, EP.E, EP.A, 6, K, K) and tuple(ego.state.shape) == (2, EP.E, 7) + HW
        # ego_masked_ref's episodes end after 9, 10 and 13 steps first: an odd cycle across two lazy resets,
        # then an even one across the third
        assert sorted(M.episode_trace(EP)["length"])[:3] == [9, 10, 13]
        for call, n in enumerate((11, 4)):
            cf, rf = (t.clone() for t in full.cycle(ag_f, 0.0, n))
            ce, re = (t.clone() for t in ego.cycle(ag_e, 0.0, n))
            torch.cuda.synchronize()
            assert cf.any(), f"cycle {call}: no lazy reset inside the cycle"
            assert torch.equal(cf, ce) and torch.equal(rf, re), f"cycle {call}: completed / returns"
            for k in CYCLE_SAME:
                assert torch.equal(getattr(full, k), getattr(ego, k)), f"cycle {call}: {k}"
            assert full.cur == ego.cur and torch.equal(rep_f.cursor, rep_e.cursor)
            size = rep_e.position()[1]
            assert size == EP.E * (11 if call == 0 else 15)
            for k in JOINT_SAME:
                assert torch.equal(getattr(rep_f, k)[:size], getattr(rep_e, k)[:size]), f"cycle {call}: ring {k}"
            for k in ("observations", "next_observations"):
                assert raw(getattr(rep_e, k)[:size]).tobytes() == crop(getattr(rep_f, k)[:size]).tobytes(), \
                    f"cycle {call}: ring {k} are not the crops of the twin's"
            assert raw(ego.obs).tobytes() == crop(full.obs).tobytes(), f"cycle {call}: obs"
        assert ag_e.seen[0] == (EP.E * EP.A, 6, K, K) and ag_f.seen[0] == (EP.E * EP.A, 6) + HW
    finally:
        close_all(made)


def test_cycle_collector_with_windows_graph_equals_eager():
    made = [make_cycle(100, ego_radius=R), make_cycle(100, ego_radius=R)]
    try:
        (_, ag_a, eager, rep_a), (_, ag_b, graphed, rep_b) = made
        n, reset = 5, False   # an odd cycle ends on the other slot, which has a graph of its own
        for call in range(4):   # 0: eager + capture (slot 0); 1: capture (slot 1) + replay; 2, 3: replays
            ca, ra = (t.clone() for t in eager.cycle(ag_a, 0.0, n))
            cb, rb = (t.clone() for t in graphed.cycle(ag_b, 0.0, n, graph=True))
            torch.cuda.synchronize()
            reset |= bool(ca.any())
            assert torch.equal(ca, cb) and torch.equal(ra, rb), f"cycle {call}: completed / returns"
            for k in CYCLE_SAME:
                assert torch.equal(getattr(eager, k), getattr(graphed, k)), f"cycle {call}: {k}"
            assert eager.cur == graphed.cur == ((call + 1) * n) & 1
            assert raw(eager.obs).tobytes() == raw(graphed.obs).tobytes(), f"cycle {call}: obs"
            for k in JOINT_SAME + ("observations", "next_observations", "cursor"):
                a, b = getattr(rep_a, k), getattr(rep_b, k)
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"cycle {call}: ring {k}"
        assert reset and graphed.captured_graphs() == {0: n, 1: n}
    finally:
        close_all(made)


def test_cycle_collector_default_is_the_full_map_path():
    made = [make_cycle(100), make_cycle(100, ego_radius=None)]
    try:
        (_, ag_a, a, rep_a), (_, ag_b, b, rep_b) = made
        a.cycle(ag_a, 0.0, 11)
        b.cycle(ag_b, 0.0, 11)
        torch.cuda.synchronize()
        for k in CYCLE_SAME + ("obs", "cycle_completed", "cycle_completed_return"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        for k in JOINT_SAME + ("observations", "next_observations", "cursor"):
            assert torch.equal(getattr(rep_a, k), getattr(rep_b, k)), k
        assert a.cycle_completed.any()
    finally:
        close_all(made)


# ---------------------------------------------------------------- refusals
def test_a_replay_of_the_wrong_obs_shape_is_refused():
    from marl_gpu.idq_rollout import IdqCollector
    from marl_gpu.qmix_cycle import QmixCycleCollector
    from marl_gpu.replay import JointReplay, TransitionReplay
    env = episode_env()
    try:
        whole, win = (6,) + HW, (6, K, K)
        with pytest.raises(ValueError, match=r"\(6, 5, 5\)"):
            IdqCollector(env, TransitionReplay(8, whole), ego_radius=R)
        with pytest.raises(ValueError, match=r"\(6, 10, 10\)"):
            IdqCollector(env, TransitionReplay(8, win))
        with pytest.raises(ValueError, match=r"\(6, 5, 5\)"):
            QmixCycleCollector(env, JointReplay(8, EP.A, whole, (7,) + HW), ego_radius=R)
        with pytest.raises(ValueError, match=r"\(6, 10, 10\)"):
            QmixCycleCollector(env, JointReplay(8, EP.A, win, (7,) + HW))
        with pytest.raises(ValueError, match=r"\(6, 7, 7\)"):
            IdqCollector(env, TransitionReplay(8, win), ego_radius=3)
        for bad in (0, 16, 2.0):
            with pytest.raises(ValueError, match="radius"):
                IdqCollector(env, TransitionReplay(8, win), ego_radius=bad)
            with pytest.raises(ValueError, match="radius"):
                QmixCycleCollector(env, JointReplay(8, EP.A, win, (7,) + HW), ego_radius=bad)
        IdqCollector(env, TransitionReplay(8, win), ego_radius=R)
        QmixCycleCollector(env, JointReplay(8, EP.A, win, (7,) + HW), ego_radius=R)
    finally:
        env.close()
