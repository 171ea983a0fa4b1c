"""The batched greedy agent (csrc/mdl_greedy.hip) against the oracle's agent at every shape edge of
greedy_matrix.py: after reset() + greedy_init() and after every greedy_actions* call the device's
moves and ops equal OracleGreedy's for every env, and the agent record a checkpoint carries (n, flags,
target, prev_carry, list[:n], free[:n]) equals OracleGreedy.record(); the same actions then step both
sides.  Three driving forms per case (full batch with auto-reset and per-episode re-initialisation,
a permuted id list of odd length, the masked form with step_episode), a checkpoint round trip into a
fresh engine for P128 and MIX, and greedy_init's refusal of a map of more than 4,096 cells.
test_greedy_matrix_cpu.py pins, on the oracle alone, what each case reaches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import greedy_matrix as M  # noqa: E402
import oracle as O  # noqa: E402

IDS = [c.id for c in M.CASES]


class Dev:
    """The device side of a case.  ``plain`` given: the engine as constructed (for load_state), with
    that many checkpoint bytes before the agents' records."""

    def __init__(self, case, plain=None):
        import marl_gpu as mg
        self.case = case
        grids = M.case_grids(case)
        self.mixed = len({g.shape for g in grids}) > 1
        self.env = mg.BatchedEnv(grids if len(grids) > 1 else grids[0], case.E, case.A, case.P, case.T,
                                 seeds=[case.seed + e for e in range(case.E)],
                                 env_map=None if len(grids) == 1 else list(case.env_map), tracker="fresh")
        self.plain = plain
        if plain is None:
            self.env.reset()
            self.plain = self.env.save_state().nbytes      # a checkpoint without the agents' records
            self.env.greedy_init()

    def cuda(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.env.device)

    def rows(self):
        c = self.case
        blob = self.env.save_state()
        assert blob.nbytes == self.plain + c.E * M.record_layout(c.A, c.P)["stride"], "the records' stride"
        return M.record_rows(blob, c.E, c.A, c.P).copy()

    def check(self, side, where, envs=None, rows=None):
        c = self.case
        rows = self.rows() if rows is None else rows
        for e in range(c.E) if envs is None else envs:
            M.assert_record(rows[e], side.record(e), c.A, c.P, f"env {e}, {where}")
        return rows

    # run_full's device side
    def actions(self):
        return self.env.greedy_actions().cpu().numpy()

    def step(self, codes):
        _, _, d = self.env.step(self.cuda(codes, np.uint8), auto_reset=True, action_format="codes")
        return d.cpu().numpy().astype(bool)

    def reinit(self, ids):
        self.env.greedy_init(env_ids=self.cuda(ids, np.int32))


def _same_actions(got, want, where):
    np.testing.assert_array_equal(got & 7, want & 7, err_msg=f"move, {where}")
    np.testing.assert_array_equal(got >> 3, want >> 3, err_msg=f"op, {where}")


@pytest.mark.parametrize("cid", IDS)
def test_full_batch(cid):
    """greedy_actions() + step(auto_reset=True) over two episode ends; greedy_init(env_ids=<done envs>)
    after each, with the oracle's agent re-made."""
    c = M.BY_ID[cid]
    side, dev = M.OracleSide(c), Dev(c)
    dev.check(side, "after greedy_init")
    M.run_full(side, 2 * c.T + 3, dev)
    dev.env.close()


@pytest.mark.parametrize("cid", IDS)
def test_id_lists(cid):
    """A permuted subset of odd length (w != e, a partial last workgroup) through
    greedy_actions(env_ids=...), step(env_ids=...) and greedy_init(env_ids=...); the envs left out keep
    their records byte for byte."""
    c = M.BY_ID[cid]
    side, dev = M.OracleSide(c), Dev(c)
    rs = np.random.RandomState(c.seed)
    n = (c.E - 3) | 1
    ids = rs.permutation(c.E)[:n]
    if (ids == np.arange(n)).all():
        ids = ids[::-1].copy()
    assert n % 2 == 1 and (ids != np.arange(n)).any()
    out = np.setdiff1d(np.arange(c.E), ids)
    ids_t = dev.cuda(ids, np.int32)
    rows0 = dev.check(side, "after greedy_init")
    for k in range(c.T + 5):                                 # past one episode end
        want = np.stack([side.actions(e) for e in ids])
        got = dev.env.greedy_actions(env_ids=ids_t).cpu().numpy()
        for w, e in enumerate(ids):
            _same_actions(got[w], want[w], f"env {e} (row {w}) step {k}")
        rows = dev.check(side, f"step {k}", envs=ids)
        assert np.array_equal(rows[out], rows0[out]), f"an env left out changed its record at step {k}"
        done = np.array([side.step(e, want[w], True) for w, e in enumerate(ids)])
        _, _, d = dev.env.step(dev.cuda(want, np.uint8), env_ids=ids_t, auto_reset=True, action_format="codes")
        np.testing.assert_array_equal(d.cpu().numpy().astype(bool), done, err_msg=f"done, step {k}")
        if done.any():
            dev.reinit(ids[done])
            rows = dev.check(side, f"re-initialised after step {k}", envs=ids)
            assert np.array_equal(rows[out], rows0[out])
    dev.check(side, "the envs left out, at the end", envs=out)
    dev.env.close()


@pytest.mark.parametrize("cid", IDS)
def test_masked(cid):
    """greedy_actions_masked(active) + step_episode over one episode: the mask is the running-episode
    mask with env 1 masked out by hand from step 0.  A masked env's row is all zero and its record is
    untouched.  (step_episode takes one map shape; the MIX engine steps its running envs by id list,
    and the test clears the finished envs' bytes itself.)"""
    c = M.BY_ID[cid]
    side, dev = M.OracleSide(c), Dev(c)
    env, hand = dev.env, 1
    active = torch.ones(c.E, dtype=torch.uint8, device=env.device)
    active[hand] = 0
    acts = torch.full((c.E, c.A), 255, dtype=torch.uint8, device=env.device)
    prev = dev.check(side, "after greedy_init")
    for k in range(c.T):
        run = active.cpu().numpy().astype(bool)
        if not run.any():
            break
        env.greedy_actions_masked(active, out=acts)
        a = acts.cpu().numpy()
        ids = np.nonzero(run)[0]
        want = {e: side.actions(e) for e in ids}
        for e in ids:
            _same_actions(a[e], want[e], f"env {e} step {k}")
        assert not a[~run].any(), f"a masked env's row is not all zero at step {k}"
        rows = dev.check(side, f"step {k}", envs=ids)
        assert np.array_equal(rows[~run], prev[~run]), f"a masked env's record changed at step {k}"
        prev = rows
        done = np.array([side.step(e, want[e], False) for e in ids])
        if dev.mixed:
            _, _, d = env.step(acts[dev.cuda(ids, np.int64)], env_ids=dev.cuda(ids, np.int32), auto_reset=False,
                               action_format="codes")
            d = d.cpu().numpy().astype(bool)
            active[dev.cuda(ids[d], np.int64)] = 0
        else:
            _, _, d, _ = env.step_episode(acts, active, action_format="codes", which=())
            d = d.cpu().numpy().astype(bool)
            assert not d[~run].any()
            d = d[run]
        np.testing.assert_array_equal(d, done, err_msg=f"done, step {k}")
    assert not active.any(), "every running episode ended within T steps"
    assert np.array_equal(dev.rows()[hand], prev[hand])
    dev.check(side, "the env masked out by hand, at the end", envs=[hand])
    env.close()


@pytest.mark.parametrize("cid", ["P128", "MIX"])
def test_checkpoint_round_trip(cid):
    """save_state mid-episode, load_state into a fresh engine: the fresh engine continues action for
    action, and record for record, with the oracle -- over the next episode end too."""
    c = M.BY_ID[cid]
    side, dev = M.OracleSide(c), Dev(c)
    k0 = c.T // 2
    M.run_full(side, k0, dev)
    blob = dev.env.save_state()
    fresh = Dev(c, plain=dev.plain)
    fresh.env.load_state(blob)
    dev.env.close()
    fresh.check(side, "after load_state")
    M.run_full(side, c.T - k0 + 5, fresh, first=k0)
    fresh.env.close()


def test_greedy_init_refuses_a_map_past_4096_cells():
    """mdl_greedy_init's refusal of a map whose BFS tables would not fit (mdl_create takes maps of up
    to 16,384 cells): the message names the map, the engine stays usable and has no agents.  The
    other refusal, the LDS budget, takes P > 1,799, which mdl_create already refuses (P <= 1,024)."""
    import marl_gpu as mg
    g = np.zeros((65, 64), np.uint8)
    E, A, P, T = 3, 2, 3, 10
    env = mg.BatchedEnv(g, E, A, P, T, seeds=[7, 8, 9], tracker="fresh")
    env.reset()
    plain = env.save_state().nbytes
    for ids in (None, torch.tensor([1], dtype=torch.int32, device=env.device)):
        with pytest.raises(mg.MdlError, match=r"mdl_greedy_init: map 0 has 4160 cells \(the BFS tables need <= 4096\)"):
            env.greedy_init(env_ids=ids)
    with pytest.raises(mg.MdlError, match="call mdl_greedy_init first"):
        env.greedy_actions()
    assert env.save_state().nbytes == plain
    envs = []
    for s in (7, 8, 9):
        o = O.OracleEnv(g, A, P, T, seed=s)
        o.reset()
        envs.append(o)
    rs = np.random.RandomState(1)
    for k in range(T):
        mv, op = rs.randint(0, 5, size=(E, A)).astype(np.uint8), rs.randint(0, 3, size=(E, A)).astype(np.uint8)
        r, _, d = env.step(torch.from_numpy(mv | (op << 3)).to(env.device), auto_reset=False, action_format="codes")
        want = [o.step(mv[e], op[e]) for e, o in enumerate(envs)]
        assert r.cpu().tolist() == [w[0] for w in want] and d.cpu().numpy().astype(bool).tolist() == [w[2] for w in want]
    s = {k: v.cpu().numpy() for k, v in env.read_state().items()}
    for e, o in enumerate(envs):
        np.testing.assert_array_equal(s["robots"][e], o.state()["robots"])
        np.testing.assert_array_equal(s["pkgs"][e], o.state()["pkgs"])
    env.close()
