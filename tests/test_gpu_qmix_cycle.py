"""Device-resident map-QMIX cycle collection: the masked lazy reset (``BatchedEnv.cycle_begin``)
against ``clear_tracker`` + ``reset`` + ``build_obs_alt`` on a twin engine; the whole cycle
(qmix/trainer.py:329-393) against its restatement on the CPU oracle; the joint replay append
(``JointReplay.add``) against the reference's sequential ``ReplayBuffer.add`` restated in numpy;
the selection that reports the exploring rows against the Philox restatement; and
``QmixCycleCollector`` against a hand-written loop over the public pieces and against its own
hipGraph replay.  Everything is compared bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from golden_io import grid  # noqa: E402
from qmix_cycle_ref import CASES, DELIVERING, NumpyJointRing, counts, oracle_cycle  # noqa: E402
from test_gpu_qmix_collect import _selection_inputs, philox4, ref_select  # noqa: E402

NAN_BITS = np.uint32(0x7FC00BAD)   # a quiet NaN no builder writes: the "row not written" sentinel
CFG = {"map": ("map.txt", 3, 6, 10, 6),       # HW = 49: the general emit path, scalar ring rows
       "map1": ("map1.txt", 5, 20, 12, 9),    # fast emit, vector ring rows, E not a multiple of 4
       "map2": ("map2.txt", 3, 70, 14, 7)}    # two package chunks


def bits(t):
    """Bit pattern of a float tensor / array as a numpy integer array (-0.0 != 0.0, NaNs compare)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    return bits(a).tobytes() == bits(b).tobytes()


def nan_filled(shape):
    return torch.from_numpy(np.full(shape, NAN_BITS, np.uint32).view(np.float32)).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_env(mg, cfg, tracker, seed):
    """The trainer's constructor: the tracker is empty when the first reset fills it."""
    mapname, A, P, T, E = cfg
    env = mg.BatchedEnv(grid(mapname), E, A, P, T, seed=seed, tracker=tracker)
    if tracker != "fresh":
        env.clear_tracker()
    env.reset()
    return env


# ------------------------------------------------- 1. cycle_begin against the existing entry points
def masks(E):
    mixed = np.zeros(E, np.uint8)
    mixed[[0, 2, E - 2]] = 1
    last = np.zeros(E, np.uint8)
    last[E - 1] = 1
    return {"none": np.zeros(E, np.uint8), "mixed": mixed, "all": np.ones(E, np.uint8), "last": last}


def check_cycle_begin(cfg, tracker, mask, state_shape=None):
    import marl_gpu
    mapname, A, P, T, E = cfg
    H, W = grid(mapname).shape
    shape = (7, H, W) if state_shape is None else state_shape
    a, b = make_env(marl_gpu, cfg, tracker, 77), make_env(marl_gpu, cfg, tracker, 77)
    rs = np.random.RandomState(5)
    for _ in range(8):
        acts = dev(rs.randint(0, 15, size=(E, A)).astype(np.uint8))
        a.step(acts, auto_reset=False)
        b.step(acts, auto_reset=False)
    before = b.read_state()
    t0, tot0 = before["t"].cpu().numpy().copy(), before["total_reward"].cpu().numpy().copy()
    assert (t0 == 8).all() and tot0.any()

    done = dev(mask)
    out = dict(idq_obs=nan_filled((E, A, 6, H, W)), qmix_state=nan_filled((E,) + shape))
    completed = torch.full((E,), 0xA5, dtype=torch.uint8, device="cuda")
    c_ret = torch.full((E,), -7.5, dtype=torch.float64, device="cuda")
    c_steps = torch.full((E,), -3, dtype=torch.int32, device="cuda")
    got = a.cycle_begin(done, out=out, completed=completed, completed_return=c_ret, completed_steps=c_steps,
                        state_shape=state_shape)
    assert got is out

    ids = np.nonzero(mask)[0]
    b.clear_tracker(ids.tolist())
    b.reset(ids.tolist())
    alt = b.build_obs_alt(state_shape=state_shape)

    assert a.save_state().tobytes() == b.save_state().tobytes(), "engine state != clear_tracker + reset"
    on, off = mask.astype(bool), ~mask.astype(bool)
    for k in ("idq_obs", "qmix_state"):
        assert same(bits(out[k])[on], bits(alt[k])[on]), f"{k}: marked rows != build_obs_alt"
        assert (bits(out[k])[off] == NAN_BITS).all(), f"{k}: rows of unmarked envs were written"
    np.testing.assert_array_equal(completed.cpu().numpy(), mask)
    assert same(c_ret, np.where(on, tot0, 0.0)), "completed_return"
    np.testing.assert_array_equal(c_steps.cpu().numpy(), np.where(on, t0, 0).astype(np.int32))
    assert not done.cpu().numpy().any(), "the mask is consumed"
    a.close()
    b.close()


@pytest.mark.parametrize("mask", ["none", "mixed", "all", "last"])
@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
@pytest.mark.parametrize("name", sorted(CFG))
def test_cycle_begin_equals_clear_reset_build(name, tracker, mask):
    check_cycle_begin(CFG[name], tracker, masks(CFG[name][4])[mask])


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
@pytest.mark.parametrize("name", ["map", "map1"])
def test_cycle_begin_other_state_shape(name, tracker):
    H, W = grid(CFG[name][0]).shape
    check_cycle_begin(CFG[name], tracker, masks(CFG[name][4])["mixed"], state_shape=(7, H + 3, W - 2))


def test_cycle_begin_null_outputs_and_refusals():
    import marl_gpu
    cfg = CFG["map1"]
    E = cfg[4]
    a, b = make_env(marl_gpu, cfg, "fresh", 3), make_env(marl_gpu, cfg, "fresh", 3)
    done = dev(masks(E)["mixed"])
    a.cycle_begin(done)                                   # every output NULL: the reset alone
    ids = np.nonzero(masks(E)["mixed"])[0].tolist()
    b.reset(ids)
    assert a.save_state().tobytes() == b.save_state().tobytes() and not done.cpu().numpy().any()
    with pytest.raises(TypeError):
        a.cycle_begin(done.to(torch.int32))
    with pytest.raises(ValueError):
        a.cycle_begin(done[:E - 1].contiguous())
    with pytest.raises(ValueError, match="must not be the done mask"):
        a.cycle_begin(done, completed=done)
    with pytest.raises(marl_gpu.MdlError, match="bad state tensor shape"):
        a.cycle_begin(done, out=dict(qmix_state=nan_filled((E, 7, 5000, 1))), state_shape=(7, 5000, 1))
    a.close()
    b.close()


# ------------------------------------------------- 2. the cycle against the oracle
@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cycle_vs_oracle(name, tracker):
    import marl_gpu
    from marl_gpu.qmix_cycle import JointReplay
    case = CASES[name]
    mapname, A, P, T, E = case["cfg"]
    H, W = grid(mapname).shape
    env = make_env(marl_gpu, case["cfg"], tracker, case["seed"])
    capacity = 101                                         # the ring wraps inside a step
    rep = JointReplay(capacity, A, (6, H, W), (7, H, W), device="cuda")
    ring = NumpyJointRing(capacity, A, (6, H, W), (7, H, W))
    obs = nan_filled((2, E, A, 6, H, W))
    state = nan_filled((2, E, 7, H, W))
    env.build_obs_alt(out={"idq_obs": obs[0], "qmix_state": state[0]})
    done = torch.zeros(E, dtype=torch.uint8, device="cuda")
    r_env = torch.zeros(E, dtype=torch.float64, device="cuda")
    r_sh = torch.zeros(E, dtype=torch.float32, device="cuda")
    completed = torch.zeros(E, dtype=torch.uint8, device="cuda")
    c_ret = torch.zeros(E, dtype=torch.float64, device="cuda")
    c_steps = torch.zeros(E, dtype=torch.int32, device="cuda")
    cur, recs = 0, []
    for rec in oracle_cycle(case):
        k = rec["k"]
        for e in case["marks"].get(k, ()):
            done[e] = 1
        env.cycle_begin(done, out={"idq_obs": obs[cur], "qmix_state": state[cur]}, completed=completed,
                        completed_return=c_ret, completed_steps=c_steps)
        np.testing.assert_array_equal(completed.cpu().numpy().astype(bool), rec["marked"], err_msg=f"step {k}: completed")
        assert same(c_ret, rec["completed_return"]), f"step {k}: completed_return"
        np.testing.assert_array_equal(c_steps.cpu().numpy(), rec["completed_steps"], err_msg=f"step {k}: steps")
        np.testing.assert_array_equal(obs[cur].cpu().numpy(), rec["obs"], err_msg=f"step {k}: obs")
        np.testing.assert_array_equal(state[cur].cpu().numpy(), rec["state"], err_msg=f"step {k}: state")
        acts = dev(rec["ints"])
        env.step(acts, auto_reset=False, out=(r_env, r_sh, done))
        assert same(r_env, rec["r_env"]), f"step {k}: r_env {r_env.cpu().numpy()} != {rec['r_env']}"
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rec["done"], err_msg=f"step {k}: done")
        env.build_obs_alt(out={"idq_obs": obs[1 - cur], "qmix_state": state[1 - cur]})
        np.testing.assert_array_equal(obs[1 - cur].cpu().numpy(), rec["next_obs"], err_msg=f"step {k}: next_obs")
        np.testing.assert_array_equal(state[1 - cur].cpu().numpy(), rec["next_state"], err_msg=f"step {k}: next_state")
        rep.add(state[cur], state[1 - cur], obs[cur], obs[1 - cur], acts, r_env, done)
        ring.add_step(rec["state"], rec["next_state"], rec["obs"], rec["next_obs"], rec["ints"], rec["r_env"], rec["done"])
        cur = 1 - cur
        recs.append(rec)
    assert_ring_equal(rep, ring, name)
    assert ring.size == capacity
    got = counts(recs, E)
    assert got == case["counts"]
    # not a quiet run: a mixed step, a step with no reset, a reset at t = T (and see CASES on deliveries)
    assert got[0] >= 1 and got[1] >= 1 and got[2] >= 1 and (got[3] >= 1 or name not in DELIVERING)
    env.close()


# ------------------------------------------------- 3. the joint replay append
def assert_ring_equal(rep, ref, what):
    assert rep.position() == (ref.ptr, ref.size), f"{what}: cursor {rep.position()} != {(ref.ptr, ref.size)}"
    for k in ("states", "next_states", "observations", "next_observations", "total_reward"):
        assert same(getattr(rep, k), getattr(ref, k)), f"{what}: {k}"
    np.testing.assert_array_equal(rep.actions.cpu().numpy(), ref.actions, err_msg=f"{what}: actions")
    np.testing.assert_array_equal(rep.dones.cpu().numpy().astype(bool), ref.dones, err_msg=f"{what}: dones")


def joint_step(k, E, A, obs_row, state_row, rs):
    """Distinct values per (step, env, agent, column): a misplaced row cannot compare equal."""
    ids = (k * E + np.arange(E)).astype(np.float64)
    state = (ids[:, None] * 64 + np.arange(state_row)).astype(np.float32)
    obs = ((ids[:, None, None] * 8 + np.arange(A)[None, :, None]) * 64 + np.arange(obs_row)).astype(np.float32)
    reward = ids * 0.1 + 1e-9                      # not float32 values: the append rounds once
    actions = ((np.arange(E * A).reshape(E, A) + 7 * k) % 251).astype(np.uint8)
    done = (rs.rand(E) < 0.3).astype(np.uint8)
    return state, state + np.float32(0.25), obs, obs + np.float32(0.5), actions, reward, done


@pytest.mark.parametrize("capacity", [64, 31, 5])
@pytest.mark.parametrize("rows", [(6, 7), (8, 12)], ids=["scalar-rows", "vector-rows"])
def test_joint_append_vs_sequential_adds(rows, capacity):
    from marl_gpu.qmix_cycle import JointReplay
    E, A = 9, 3
    obs_row, state_row = rows
    assert ((A * obs_row) % 4 == 0 and state_row % 4 == 0) == (rows == (8, 12))
    rep = JointReplay(capacity, A, (obs_row,), (state_row,), device="cuda")
    ref = NumpyJointRing(capacity, A, (obs_row,), (state_row,))
    rs = np.random.RandomState(obs_row * 100 + capacity)
    for k in range(10):
        x = joint_step(k, E, A, obs_row, state_row, rs)
        rep.add(*(dev(v) for v in x))
        ref.add_step(*x)
        assert_ring_equal(rep, ref, f"rows {rows} capacity {capacity} step {k}")
    assert ref.size == capacity


def test_joint_append_unaligned_rows_take_the_scalar_path():
    """Vector-sized rows from a tensor whose storage starts 4 bytes off a 16-byte boundary."""
    from marl_gpu.qmix_cycle import JointReplay
    E, A, obs_row, state_row, capacity = 9, 3, 8, 12, 31
    rep = JointReplay(capacity, A, (obs_row,), (state_row,), device="cuda")
    ref = NumpyJointRing(capacity, A, (obs_row,), (state_row,))
    rs = np.random.RandomState(5)
    for k in range(5):
        x = joint_step(k, E, A, obs_row, state_row, rs)
        d = [dev(v) for v in x]
        which = k % 4                                        # state, next_state, obs, next_obs in turn
        off = torch.zeros(x[which].size + 1, dtype=torch.float32, device="cuda")[1:].view(x[which].shape)
        off.copy_(d[which])
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        d[which] = off
        rep.add(*d)
        ref.add_step(*x)
        assert_ring_equal(rep, ref, f"step {k}")


def test_joint_append_checks_its_arguments():
    from marl_gpu.qmix_cycle import JointReplay
    rep = JointReplay(8, 3, (4,), (4,), device="cuda")
    x = [dev(v) for v in joint_step(0, 5, 3, 4, 4, np.random.RandomState(0))]
    with pytest.raises(TypeError):
        rep.add(x[0], x[1], x[2], x[3], x[4], x[5].float(), x[6])
    with pytest.raises(ValueError):
        rep.add(x[0][:4].contiguous(), x[1], x[2], x[3], x[4], x[5], x[6])
    assert rep.position() == (0, 0)


# ------------------------------------------------- 4. the selection that reports the exploring rows
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
def test_marked_selection(eps):
    from marl_gpu import qmix_cycle as QC, qmix_rollout as Q
    N = 4096
    q, avail = _selection_inputs(N)
    seed, off = 0x0123_4567_89AB_CDEF, (5 << 32) + 11
    qd, ad = dev(q), dev(avail)
    plain = Q.select_actions_eps(qd, eps, seed, off, avail=ad).cpu().numpy()
    got, explored = QC.select_actions_eps_mark(qd, eps, seed, off, avail=ad)
    np.testing.assert_array_equal(got.cpu().numpy(), plain)
    want, explore = ref_select(q, avail, eps, seed, off)
    np.testing.assert_array_equal(plain, want)
    np.testing.assert_array_equal(explored.cpu().numpy(), (explore & avail.any(1)).astype(np.uint8))
    assert (explored.cpu().numpy()[:64] == 0).all()                      # no available action: never explored
    if eps == 0.0:
        assert not explored.any()
    elif eps == 1.0:
        assert explored.cpu().numpy()[64:].all()
    else:
        assert 0 < int(explored.sum()) < N
    # no mask = every action available; the explore bit is the float32 compare of the header
    x0 = philox4(np.full(N, off & 0xFFFFFFFF), np.full(N, off >> 32), np.arange(N), np.zeros(N), seed & 0xFFFFFFFF,
                 seed >> 32)[0]
    u = (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    gn, en = QC.select_actions_eps_mark(qd, eps, seed, off)
    np.testing.assert_array_equal(en.cpu().numpy(), (u < np.float32(eps)).astype(np.uint8))
    np.testing.assert_array_equal(gn.cpu().numpy(), Q.select_actions_eps(qd, eps, seed, off).cpu().numpy())
    # the device-argument form at the same values
    eps_dev = torch.tensor([eps], dtype=torch.float32, device="cuda")
    off_dev = torch.tensor([off - 1000], dtype=torch.int64, device="cuda")
    gd, ed = QC.select_actions_eps_mark_dev(qd, eps_dev, seed, off_dev, 1000, avail=ad)
    np.testing.assert_array_equal(gd.cpu().numpy(), plain)
    np.testing.assert_array_equal(ed.cpu().numpy(), explored.cpu().numpy())
    np.testing.assert_array_equal(Q.select_actions_eps_dev(qd, eps_dev, seed, off_dev, 1000, avail=ad).cpu().numpy(), plain)


# ------------------------------------------------- 5. / 6. the collector
COLLECT = dict(cfg=CFG["map1"], env_seed=300, agent_seed=5, seed=13, capacity=101, hidden=16)


class GruAgent(torch.nn.Module):
    """A small recurrent Q network: a GRU cell written out of Linear layers."""

    def __init__(self, H, W, hidden):
        super().__init__()
        L = torch.nn.Linear
        self.enc, self.gi, self.gh, self.out = L(6 * H * W, hidden), L(hidden, 3 * hidden), L(hidden, 3 * hidden), L(hidden, 15)
        g = torch.Generator().manual_seed(COLLECT["agent_seed"])
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)

    def forward(self, obs, hidden):
        x = torch.relu(self.enc(obs.flatten(1)))
        i_r, i_z, i_n = self.gi(x).chunk(3, 1)
        h_r, h_z, h_n = self.gh(hidden).chunk(3, 1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        h = (1.0 - z) * torch.tanh(i_n + r * h_n) + z * hidden
        return self.out(h), h


def make_collector(mg, tracker="fresh"):
    from marl_gpu.qmix_cycle import JointReplay, QmixCycleCollector
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    H, W = grid(mapname).shape
    env = mg.BatchedEnv(grid(mapname), E, A, P, T, seed=c["env_seed"], tracker=tracker)
    rep = JointReplay(c["capacity"], A, (6, H, W), (7, H, W), device="cuda")
    return env, rep, QmixCycleCollector(env, rep, seed=c["seed"], hidden_dim=c["hidden"])


def explore_mask(eps, seed, offset, N):
    x0 = philox4(np.full(N, offset & 0xFFFFFFFF), np.full(N, offset >> 32), np.arange(N), np.zeros(N),
                 seed & 0xFFFFFFFF, seed >> 32)[0]
    return (x0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) < np.float32(eps)


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
def test_collector_equals_hand_written_loop(tracker):
    import marl_gpu
    from marl_gpu.qmix_rollout import select_actions_eps
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    H, W = grid(mapname).shape
    Hd, eps = c["hidden"], 0.3
    env, rep, col = make_collector(marl_gpu, tracker)
    agent = GruAgent(H, W, Hd).cuda()
    agent.train()
    col.begin()
    n1, n2, forced = T + 3, 7, [2, 5]                      # the first cycle passes the time limit
    comp1, ret1 = (x.clone() for x in col.cycle(agent, eps, n1))
    assert agent.training                                  # the mode is restored
    col.done[forced] = 1                                   # two episodes cut between the cycles
    comp2, ret2 = (x.clone() for x in col.cycle(agent, eps, n2))
    assert col.offset == n1 + n2 and comp1.shape == (n1, E) and comp2.shape == (n2, E)

    ref = make_env(marl_gpu, c["cfg"], tracker, c["env_seed"])
    ring = NumpyJointRing(c["capacity"], A, (6, H, W), (7, H, W))
    agent.eval()
    obs = torch.zeros((2, E, A, 6, H, W), dtype=torch.float32, device="cuda")
    state = torch.zeros((2, E, 7, H, W), dtype=torch.float32, device="cuda")
    ref.build_obs_alt(out={"idq_obs": obs[0], "qmix_state": state[0]})
    hidden = torch.zeros((E * A, Hd), dtype=torch.float32, device="cuda")
    done = np.zeros(E, bool)
    u = torch.zeros((E, A), dtype=torch.uint8, device="cuda")
    offset, cur, kept, zeroed = 0, 0, 0, 0
    with torch.no_grad():
        for n_steps, comp, ret in ((n1, comp1, ret1), (n2, comp2, ret2)):
            if n_steps == n2:
                done[forced] = True
            for k in range(n_steps):
                ids = np.nonzero(done)[0]
                st = ref.read_state()
                want_ret = np.where(done, st["total_reward"].cpu().numpy(), 0.0)
                np.testing.assert_array_equal(comp[k].cpu().numpy().astype(bool), done, err_msg=f"step {k}: completed")
                assert same(ret[k], want_ret), f"step {k}: completed_return"
                if ids.size:
                    ref.clear_tracker(ids.tolist())
                    ref.reset(ids.tolist())
                    ref.build_obs_alt(out={"idq_obs": obs[cur], "qmix_state": state[cur]})
                    hidden.view(E, A, Hd)[torch.from_numpy(ids).cuda()] = 0.0
                    zeroed += ids.size
                    done[:] = False
                q, new_hidden = agent(obs[cur].reshape(E * A, 6, H, W), hidden)
                select_actions_eps(q, eps, c["seed"], offset, out=u.view(-1))     # the unmarked entry point
                ex = explore_mask(eps, c["seed"], offset, E * A)
                kept += int(ex.sum())
                hidden = torch.where(torch.from_numpy(ex).cuda().unsqueeze(1), hidden, new_hidden)
                offset += 1
                r, _, d = ref.step(u, auto_reset=False)
                ref.build_obs_alt(out={"idq_obs": obs[1 - cur], "qmix_state": state[1 - cur]})
                ring.add_step(state[cur].cpu().numpy(), state[1 - cur].cpu().numpy(), obs[cur].cpu().numpy(),
                              obs[1 - cur].cpu().numpy(), u.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy())
                done = d.cpu().numpy().astype(bool)
                cur = 1 - cur
    assert_ring_equal(rep, ring, "collector vs hand-written loop")
    assert env.save_state().tobytes() == ref.save_state().tobytes(), "engine state"
    assert same(col.hidden, hidden), "hidden state"
    np.testing.assert_array_equal(col.done.cpu().numpy().astype(bool), done)
    assert col.cur == cur
    assert int(comp1.sum()) == E and int(comp2.sum()) >= len(forced)    # every env passed T once; the forced marks
    assert comp2[0].cpu().numpy()[forced].all()
    assert kept > 0 and zeroed > 0 and ring.size == c["capacity"]
    assert len(set(ring.total_reward[:, 0].tolist())) > 3, "the rewards must vary"
    env.close()
    ref.close()


@pytest.mark.parametrize("tracker", ["fresh", "mappo"])
def test_cycle_graph_replay_equals_eager(tracker):
    import marl_gpu
    c = COLLECT
    mapname, A, P, T, E = c["cfg"]
    H, W = grid(mapname).shape
    env_e, rep_e, eager = make_collector(marl_gpu, tracker)
    env_g, rep_g, graph = make_collector(marl_gpu, tracker)
    agent = GruAgent(H, W, c["hidden"]).cuda()
    eager.begin()
    graph.begin()
    n, resets = 7, 0                        # odd: the cycles alternate between the two observation slots
    for call, eps in enumerate((0.3, 0.5, 0.1)):   # the later graph calls are replays, at other epsilons
        xc, xr = (t.clone() for t in eager.cycle(agent, eps, n))
        yc, yr = (t.clone() for t in graph.cycle(agent, eps, n, graph=True))
        assert same(xc, yc) and same(xr, yr), f"call {call}: completed rows"
        assert rep_e.position() == rep_g.position(), f"call {call}: cursor"
        for k in ("states", "next_states", "observations", "next_observations", "actions", "total_reward", "dones"):
            assert same(getattr(rep_e, k), getattr(rep_g, k)), f"call {call}: {k}"
        assert env_e.save_state().tobytes() == env_g.save_state().tobytes(), f"call {call}: engine state"
        assert same(eager.hidden, graph.hidden) and same(eager.done, graph.done), f"call {call}: hidden / done"
        assert eager.offset == graph.offset == (call + 1) * n and eager.cur == graph.cur
        resets += int(yc.sum())
    assert graph.captured_graphs() == {0: n, 1: n}   # one graph per starting slot
    assert resets == E, "the calls together pass the time limit once: a replayed graph reset every env"
    env_e.close()
    env_g.close()


def test_graph_and_eager_cycles_interleave():
    """Graphed and eager ``cycle`` calls on one collector, and an assigned ``offset``, select exactly
    what eager calls alone select."""
    import marl_gpu
    from marl_gpu.qmix_cycle import JointReplay, QmixCycleCollector
    c = COLLECT
    # epsilon 0.5: about half the rows' actions depend on the offset; an odd cycle alternates the slots
    E, A, P, T, n, eps = 4, 2, 2, 20, 3, 0.5
    H, W = grid("map.txt").shape

    def make():
        env = marl_gpu.BatchedEnv(grid("map.txt"), E, A, P, T, seed=c["env_seed"], tracker="fresh")
        rep = JointReplay(13, A, (6, H, W), (7, H, W), device="cuda")   # the ring wraps during the sequence
        col = QmixCycleCollector(env, rep, seed=c["seed"], hidden_dim=c["hidden"])
        col.begin()
        return env, rep, col

    env_e, rep_e, eager = make()
    env_o, rep_o, other = make()
    agent = GruAgent(H, W, c["hidden"]).cuda()
    # capture (slot 1), replay, eager, replay, and a replay that first captures slot 0
    for call, graph in enumerate((True, True, False, True, True)):
        if call == 4:
            other.offset = eager.offset = 1000
        xc, xr = (t.clone() for t in eager.cycle(agent, eps, n))
        yc, yr = (t.clone() for t in other.cycle(agent, eps, n, graph=graph))
        assert same(xc, yc) and same(xr, yr), f"call {call}: completed rows"
        assert rep_e.position() == rep_o.position(), f"call {call}: cursor"
        for k in ("states", "next_states", "observations", "next_observations", "actions", "total_reward", "dones"):
            assert same(getattr(rep_e, k), getattr(rep_o, k)), f"call {call}: {k}"
        assert env_e.save_state().tobytes() == env_o.save_state().tobytes(), f"call {call}: engine state"
        assert same(eager.hidden, other.hidden) and same(eager.done, other.done), f"call {call}: hidden / done"
        assert same(eager.u, other.u) and same(eager.explored, other.explored), f"call {call}: actions"
        assert eager.offset == other.offset == (1000 + n if call == 4 else (call + 1) * n), f"call {call}"
        assert eager.cur == other.cur
    assert other.captured_graphs() == {0: n, 1: n}
    env_e.close()
    env_o.close()
