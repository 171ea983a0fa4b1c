"""Device-resident evaluation (marl_gpu.evaluate) on the GPU: the masked greedy agent and the
episode results against the CPU oracle and against the entry points they extend, the ``Evaluator``
for its three agent kinds (eager and as replayed hipGraphs), and ``run_eval`` against the
reference's recorded evaluation (tests/golden/eval_anchor.json, README.md:117-121)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eval_ref as R  # noqa: E402
from golden_io import grid, load_json  # noqa: E402


def _mg():
    import marl_gpu
    return marl_gpu


def _engine(name, reset=True):
    """A shape's engine.  A newly built engine holds the constructor's layout draw and the first
    ``reset()`` starts the reference's episode (Environment(seed) then env.reset(), evaluation.py:13-20);
    an ``Evaluator`` run makes that reset itself, so its engines come un-reset."""
    c = R.SHAPES[name]
    env = _mg().BatchedEnv(grid(c["mapname"]), R.E, c["A"], c["P"], c["T"], seeds=R.SEEDS, tracker="fresh")
    if reset:
        env.reset()
    return env


def _ones(env):
    return torch.ones(env.E, dtype=torch.uint8, device=env.device)


def _host_results(env):
    s = env.read_state()
    return (s["total_reward"].cpu().numpy(), (s["pkgs"][:, :, 7] == 3).sum(1).cpu().numpy(), s["t"].cpu().numpy())


def _same_results(res, rewards, delivered, steps):
    got = res["rewards"].cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), np.asarray(rewards, np.float64).view(np.uint64))
    assert res["delivered"].cpu().tolist() == [int(x) for x in delivered]
    assert res["steps"].cpu().tolist() == [int(x) for x in steps]


# ---- 1. the masked greedy agent against the oracle, over whole ragged episodes
@pytest.mark.parametrize("name", ["R3", "R9"])
def test_masked_greedy_vs_oracle(name):
    ep = R.greedy_episodes(name)
    env = _engine(name)
    env.greedy_init()
    active = _ones(env)
    acts = torch.full((env.E, env.A), 255, dtype=torch.uint8, device=env.device)
    for k in range(env.T):
        assert np.array_equal(active.cpu().numpy().astype(bool), ep["running"][k]), f"mask before step {k}"
        env.greedy_actions_masked(active, out=acts)
        a = acts.cpu().numpy()
        run = ep["running"][k]
        np.testing.assert_array_equal(a[run] & 7, ep["codes"][k][run] & 7, err_msg=f"move, step {k}")
        np.testing.assert_array_equal(a[run] >> 3, ep["codes"][k][run] >> 3, err_msg=f"op, step {k}")
        assert not a[~run].any(), f"a finished env's row is not all zero at step {k}"
        r, _, d, _ = env.step_episode(acts, active, action_format="codes", which=())
        assert np.array_equal(r.cpu().numpy().view(np.uint64), ep["r"][k].view(np.uint64)), f"reward, step {k}"
        assert np.array_equal(d.cpu().numpy().astype(bool), ep["done"][k]), f"done, step {k}"
    assert not active.any()
    _same_results(dict(zip(("rewards", "delivered", "steps"), env.episode_results())), ep["rewards"], ep["delivered"],
                  ep["steps"])
    env.close()


# ---- 2. a skipped env's agent record is untouched
def _greedy_records(env, plain_bytes):
    """The agent records of every env: the section mdl_greedy_init adds to a checkpoint, [E, stride]."""
    blob = env.save_state()
    return blob[plain_bytes:].reshape(env.E, -1)


def test_skipped_env_record_is_untouched():
    """At step 4 engine X calls the masked form with every second env masked out and discards the
    actions; a touched record would have appended that step's spawns (and re-chosen targets) twice.
    The skipped envs' records stay byte for byte those of the twin that made no such call, and their
    actions stay the twin's for 10 further steps.  The same at step 0, where every package spawns
    (get_actions at t = 0 appends them): there the envs that were NOT skipped do change their
    records, which shows the discarded call is not a no-op."""
    X, Y = _engine("R3"), _engine("R3")
    plain = X.save_state().nbytes
    skip = torch.zeros(X.E, dtype=torch.uint8, device=X.device)
    skip[1::2] = 1                                           # envs 0, 2, 4, ... are masked out
    out = (skip == 0).cpu().numpy()
    for env in (X, Y):
        env.greedy_init()
    act = {id(X): _ones(X), id(Y): _ones(Y)}

    def discarded_call():
        X.greedy_actions_masked(skip)
        rx, ry = _greedy_records(X, plain), _greedy_records(Y, plain)
        assert rx.shape == ry.shape and rx.shape[1] > 8
        assert np.array_equal(rx[out], ry[out])
        return bool((rx[~out] != ry[~out]).any())

    def step_both(k):
        ax, ay = X.greedy_actions_masked(act[id(X)]), Y.greedy_actions_masked(act[id(Y)])
        assert torch.equal(ax[::2], ay[::2]), f"a skipped env's actions differ at step {k}"
        # X's other envs ran get_actions twice in one step, so from here on they are their own episodes
        X.step_episode(ax, act[id(X)], action_format="codes", which=())
        Y.step_episode(ay, act[id(Y)], action_format="codes", which=())

    assert discarded_call(), "the discarded call at t = 0 changed no record at all"
    for k in range(4):
        step_both(k)
    discarded_call()
    for k in range(4, 15):
        step_both(k)
    sx, sy = _host_results(X), _host_results(Y)
    for a, b in zip(sx, sy):
        assert np.array_equal(a[::2], b[::2])
    X.close()
    Y.close()


# ---- 3. an all-ones mask and no mask are greedy_actions()
@pytest.mark.parametrize("mapname,A,P,T", [("map1.txt", 3, 3, 50), ("map2.txt", 8, 60, 100)])
def test_unmasked_equivalence(mapname, A, P, T):
    mg = _mg()
    envs = [mg.BatchedEnv(grid(mapname), R.E, A, P, T, seeds=R.SEEDS, tracker="fresh") for _ in range(3)]
    for env in envs:
        env.reset()
        env.greedy_init()
    a, b, c = envs
    ones = _ones(b)
    for k in range(20):
        want = a.greedy_actions()
        got_ones = b.greedy_actions_masked(ones)
        got_null = c.greedy_actions_masked(None)
        assert torch.equal(got_ones, want) and torch.equal(got_null, want), f"step {k}"
        for env, acts in ((a, want), (b, got_ones), (c, got_null)):
            env.step(acts, auto_reset=False, action_format="codes")
    blobs = [env.save_state() for env in envs]                # state and agent records, byte for byte
    assert np.array_equal(blobs[0], blobs[1]) and np.array_equal(blobs[0], blobs[2])
    for env in envs:
        env.close()


# ---- 4. episode_results against the read_state export it replaces
def test_episode_results_vs_read_state():
    mg = _mg()
    E, A, T = 5, 5, 200                                       # E = 5: the second workgroup is partial
    any_delivered = 0
    for P in (1, 63, 64, 65, 100, 300):                       # both sides of the 64-slot chunk edges
        env = mg.BatchedEnv(grid("map1.txt"), E, A, P, T, seeds=R.SEEDS[:E], tracker="fresh")
        env.reset()
        env.greedy_init()
        active = _ones(env)
        for _ in range(40):
            env.step_episode(env.greedy_actions_masked(active), active, action_format="codes", which=())
        tot, dl, st = _host_results(env)
        r, d, s = env.episode_results()
        assert r.dtype == torch.float64 and d.dtype == torch.int32 and s.dtype == torch.int32
        assert r.shape == d.shape == s.shape == (E,)
        assert np.array_equal(r.cpu().numpy().view(np.uint64), tot.view(np.uint64)), f"P={P}"
        assert d.cpu().tolist() == dl.tolist(), f"P={P}"
        assert s.cpu().tolist() == st.tolist(), f"P={P}"
        any_delivered += int(dl.sum())
        for skip in range(3):                                 # each output may be left out
            bufs = [torch.full((E,), -7, dtype=t.dtype, device=env.device) for t in (r, d, s)]
            got = env.episode_results(out=tuple(None if i == skip else b for i, b in enumerate(bufs)))
            assert got[skip] is None
            for i, want in enumerate((r, d, s)):
                if i != skip:
                    assert torch.equal(got[i], want), f"P={P}, without output {skip}"
        with pytest.raises(TypeError):
            env.episode_results(out=(r, d.long(), s))
        with pytest.raises(ValueError):
            env.episode_results(out=(r[:E - 1], d, s))
        env.close()
    assert any_delivered > 0, "no case delivered a package: the count was never non-zero"


# ---- 5. Evaluator("greedy") against the oracle's episodes, eager and as replayed graphs
@pytest.mark.parametrize("name", ["R3", "R9"])
def test_evaluator_greedy_vs_oracle(name):
    mg = _mg()
    ep = R.greedy_episodes(name)
    env = _engine(name, reset=False)
    built = env.save_state()          # every run resets, i.e. draws the next layouts: rewind the engine between runs
    ev = mg.Evaluator(env)
    res = ev.run("greedy")
    _same_results(res, ep["rewards"], ep["delivered"], ep["steps"])
    assert res["finished"].dtype == torch.uint8 and res["finished"].cpu().tolist() == [1] * env.E
    s = ev.summary()
    assert s["rewards"] == ep["rewards"].tolist() and s["delivered"] == ep["delivered"].tolist()
    assert float(s["mean_reward"]) == float(np.mean(ep["rewards"].tolist()))
    # 7 does not divide 50: seven replays of the chunk and a one-step remainder graph
    for call in range(3):                                     # eager + capture, then two replays
        ev.rewards.zero_()
        ev.delivered.zero_()
        env.load_state(built)
        _same_results(ev.run("greedy", graph=True, graph_steps=7), ep["rewards"], ep["delivered"], ep["steps"])
        assert ev.captured_graphs() == {"chunk": 7, "rest": 1}, call
    # the remainder path decides the result when the run stops before every episode is over
    env.load_state(built)
    eager = {k: v.clone() for k, v in mg.Evaluator(env).run("greedy", max_steps=20).items()}
    assert eager["steps"].cpu().tolist() == np.minimum(ep["steps"], 20).tolist()
    assert eager["finished"].cpu().tolist() == (ep["steps"] <= 20).astype(int).tolist()
    assert 0 < int(eager["finished"].sum()) < env.E
    for call in range(2):
        env.load_state(built)
        got = ev.run("greedy", max_steps=20, graph=True, graph_steps=7)
        assert ev.captured_graphs() == {"chunk": 7, "rest": 6}
        for k in eager:
            assert torch.equal(got[k], eager[k]), (k, call)
    env.close()


# ---- 6. the README anchor
def test_run_eval_readme_anchor():
    mg = _mg()
    ref = load_json("eval_anchor.json")
    cfg = ref["config"]
    env_config = dict(map=cfg["map"], max_time_steps=cfg["max_time_steps"], n_agents=cfg["n_agents"],
                      n_packages=cfg["n_packages"], seed=cfg["seed"])
    s = mg.run_eval("greedy", env_config, cfg["episodes"])
    assert s["rewards"] == ref["greedy"]["rewards"]
    assert s["delivered"] == ref["greedy"]["delivered"]
    assert float(s["mean_reward"]) == ref["greedy"]["mean_reward"]
    assert float(s["std_reward"]) == ref["greedy"]["std_reward"]
    assert float(s["mean_delivered"]) == ref["greedy"]["mean_delivered"]
    assert round(float(s["mean_reward"]), 2) == 34.04 and round(float(s["std_reward"]), 2) == 14.83
    s = mg.run_eval("random", env_config, 10)                 # an episode's draws depend only on those before it
    assert s["rewards"] == ref["random"]["rewards"][:10]
    assert s["delivered"] == ref["random"]["delivered"][:10]
    with pytest.raises(ValueError):
        mg.run_eval("nobody", env_config, 2)


# ---- 7. an action tape against the oracle
def test_tape_vs_oracle():
    mg = _mg()
    g, A, P, T, E = grid("map2.txt"), 8, 6, 30, 16
    seeds = R.SEEDS[:E]
    rs = np.random.RandomState(7)
    tape = (rs.randint(0, 5, size=(T, E, A)) | (rs.randint(0, 3, size=(T, E, A)) << 3)).astype(np.uint8)
    want = R.tape_episodes(g, A, P, T, seeds, tape)
    env = mg.BatchedEnv(g, E, A, P, T, seeds=seeds, tracker="fresh")
    built = env.save_state()          # every run resets, i.e. draws the next layouts: rewind the engine between runs
    ev = mg.Evaluator(env)
    dev_tape = torch.from_numpy(tape).to(env.device)
    _same_results(ev.run(dev_tape), *want)
    for _ in range(2):                                        # eager + capture, then a replay of all T steps
        ev.rewards.zero_()
        env.load_state(built)
        _same_results(ev.run(dev_tape, graph=True), *want)
    assert ev.captured_graphs() == {"chunk": T}
    env.load_state(built)
    _same_results(ev.run(dev_tape, max_steps=11), *R.tape_episodes(g, A, P, T, seeds, tape, max_steps=11))
    with pytest.raises(ValueError, match="needs 30"):
        ev.run(dev_tape[:T - 1])
    with pytest.raises(ValueError):
        ev.run(dev_tape[:, :E - 1].contiguous())
    env.close()


# ---- 8. a policy, against a host-driven loop written from the existing API
class _LinearActor(torch.nn.Module):
    def __init__(self, H, W, Dv, device):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.wm = torch.nn.Parameter((torch.randn(6 * H * W, 15, generator=g) * 0.3).to(device))
        self.wv = torch.nn.Parameter(torch.randn(Dv, 15, generator=g).to(device))

    def forward(self, amap, avec):
        return amap.reshape(amap.shape[0], -1) @ self.wm + avec @ self.wv


def _host_driven_policy(mg, env, policy, deterministic, seed):
    """The loop of tests/test_gpu_greedy.py::run_greedy_episodes with a policy: done read back every
    step, the id list rebuilt on the host.  The selector and the sampler key their draws by row, so
    they run on the full batch and the finished envs' rows are discarded."""
    from marl_gpu.rollout import sample_actions
    E, A = env.E, env.A
    env.reset()
    active = np.arange(E)
    k = 0
    with torch.no_grad():
        while active.size:
            obs = env.build_obs(which=("actor_map", "actor_vec"))
            logits = policy(obs["actor_map"].reshape(E * A, *obs["actor_map"].shape[2:]),
                            obs["actor_vec"].reshape(E * A, -1))
            if deterministic:
                acts = mg.select_actions_eps(logits, 0.0, seed, 0)
            else:
                acts, _ = sample_actions(logits, seed, k)
            ids = torch.from_numpy(active.astype(np.int32)).to(env.device)
            _, _, done = env.step(acts.view(E, A)[ids.long()].contiguous(), env_ids=ids, auto_reset=False)
            active = active[~done.cpu().numpy().astype(bool)]
            k += 1
    return _host_results(env)


@pytest.mark.parametrize("deterministic", [True, False])
def test_policy_vs_host_driven_loop(deterministic):
    mg = _mg()
    env = _mg().BatchedEnv(grid("map1.txt"), 16, 3, 3, 50, seeds=R.SEEDS[:16], tracker="fresh")
    H, W = env.grids[0].shape
    policy = _LinearActor(H, W, env.actor_vec_dim, env.device)
    policy.train()
    built = env.save_state()          # every run resets, i.e. draws the next layouts: rewind the engine between runs
    want = _host_driven_policy(mg, env, policy, deterministic, seed=5)
    assert int(want[2].min()) >= 1
    ev = mg.Evaluator(env, seed=5)
    env.load_state(built)
    _same_results(ev.run(policy, deterministic=deterministic), *want)
    assert policy.training                                    # eval mode inside, the mode restored
    # the sampler's offset advances from run to run: a fresh Evaluator starts at the host loop's offset 0
    ev = mg.Evaluator(env, seed=5)
    env.load_state(built)
    _same_results(ev.run(policy, deterministic=deterministic, graph=True, graph_steps=16), *want)
    assert ev.captured_graphs() == {"chunk": 16, "rest": 2}
    env.load_state(built)
    if deterministic:
        _same_results(ev.run(policy, deterministic=True, graph=True, graph_steps=16), *want)    # a replay
    else:
        # the replayed run draws at offsets 50 .. 99, as a second eager run of one Evaluator does
        two = mg.Evaluator(env, seed=5)
        two.run(policy, deterministic=False)
        env.load_state(built)
        second = {k: v.clone() for k, v in two.run(policy, deterministic=False).items()}
        env.load_state(built)
        got = ev.run(policy, deterministic=False, graph=True, graph_steps=16)
        for k in second:
            assert torch.equal(got[k], second[k]), k
        assert ev.offset == two.offset == 100
    env.close()


def test_graph_and_eager_sampled_runs_interleave():
    """Graphed and eager sampled-policy runs on one Evaluator, and an assigned ``offset``, draw exactly
    what eager runs alone draw (a three-step chunk and a one-step remainder graph per replayed run)."""
    mg = _mg()
    E, A, P, T, L = 4, 2, 2, 20, 4
    env_e, env_o = (mg.BatchedEnv(grid("map.txt"), E, A, P, T, seeds=R.SEEDS[:E], tracker="fresh") for _ in range(2))
    H, W = env_e.grids[0].shape
    policy = _LinearActor(H, W, env_e.actor_vec_dim, env_e.device)
    eager, other = mg.Evaluator(env_e, seed=5), mg.Evaluator(env_o, seed=5)
    for call, graph in enumerate((True, True, False, True, True)):   # capture, replay, eager, replay, replay
        if call == 4:
            other.offset = eager.offset = 1000
        x = {k: v.clone() for k, v in eager.run(policy, max_steps=L, deterministic=False).items()}
        y = other.run(policy, max_steps=L, deterministic=False, graph=graph, graph_steps=3)
        for k in x:
            assert torch.equal(x[k], y[k]), (call, k)
        assert torch.equal(eager.actions, other.actions), call
        assert env_e.save_state().tobytes() == env_o.save_state().tobytes(), call
        assert eager.offset == other.offset == (1000 + L if call == 4 else (call + 1) * L), call
    assert other.captured_graphs() == {"chunk": 3, "rest": 1}
    env_e.close()
    env_o.close()


# ---- 9. refusals
def test_refusals():
    mg = _mg()
    mixed = mg.BatchedEnv([grid("map1.txt"), grid("map2.txt")], 8, 5, 20, 30, seed=1, env_map=[0] * 4 + [1] * 4)
    with pytest.raises(ValueError, match="mix map shapes"):
        mg.Evaluator(mixed)
    mixed.close()
    env = mg.BatchedEnv(grid("map1.txt"), 4, 3, 3, 20, seed=1)
    env.reset()
    with pytest.raises(mg.MdlError, match="greedy_init"):
        env.greedy_actions()
    with pytest.raises(mg.MdlError, match="greedy_init"):
        env.greedy_actions_masked(_ones(env))
    env.greedy_init()
    with pytest.raises(TypeError):
        env.greedy_actions_masked(_ones(env).bool())
    with pytest.raises(ValueError):
        env.greedy_actions_masked(_ones(env)[:3])
    with pytest.raises(ValueError):
        env.greedy_actions_masked(_ones(env), out=torch.zeros(4, 2, dtype=torch.uint8, device=env.device))
    ev = mg.Evaluator(env)
    with pytest.raises(ValueError):
        ev.run("greedier")
    with pytest.raises(TypeError):
        ev.run(3)
    env.close()
