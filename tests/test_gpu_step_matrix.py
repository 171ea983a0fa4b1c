"""Every step-kernel instantiation (tests/step_matrix.py: 96 symbols, one case each) against the CPU
oracle, bit for bit after every step: fp64 env reward, float32 shaped reward, done, robots, packages,
t, total reward and the tracker rows -- through the launch variant that reaches the kernel (step,
step_fused, mail_step, step_obs, step_episode; the rows and halves layouts).

Each case first runs the oracle alone (a trace of every call's expected results) and asserts on that
trace that the inputs exercise the kernel -- a pick-up in every case, two resets of every env in
every non-episode case, a delivery in at least half of the cases of each kernel family and tracker
mode -- before the engine is stepped against it."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from golden_io import grid  # noqa: E402
from step_matrix import CASES, codes_of, n_steps, trainer_ints  # noqa: E402

OBS_KEYS = ("actor_map", "actor_vec", "critic_map", "critic_vec")
SENTINEL = -7.25    # no observation feature is negative
MP, MR, MPS = 5, 100, 100   # observation dims: max_packages_obs as the other tests pass it, the engine's defaults
EPISODE_CUTS = {1: 3, 3: 7, 0: 12}   # env -> the step its episode is cut at by the caller; the rest run to T
EPISODE_ZERO_MASK_STEP = 4           # one extra call with an all-zero mask before this step


@pytest.fixture(scope="module", autouse=True)
def _setup():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    O.build()


# ------------------------------------------------------------------ the oracle side (CPU only)
class _Oracle:
    """The case's envs: one OracleBatch over all E (full-batch calls only), or one single-env
    OracleBatch per env with seed_base = seed + e where calls step a subset."""

    def __init__(self, case, singles):
        self.g = grid(case.map)
        self.E, self.singles = case.E, singles
        kw = dict(clear_on_reset=(case.tracker == "fresh"))
        if singles:
            self.b = [O.OracleBatch(1, self.g, case.A, case.P, case.T, seed_base=case.seed + e, **kw)
                      for e in range(case.E)]
        else:
            self.b = O.OracleBatch(case.E, self.g, case.A, case.P, case.T, seed_base=case.seed, **kw)

    def _at(self, e):
        return (self.b[e], 0) if self.singles else (self.b, e)

    def step(self, ids, ints, auto_reset):
        """Step the envs `ids` (None: all, one call) with rows ints[e]; (r, sh, done) in the order of ids."""
        if ids is None:
            assert not self.singles
            return self.b.step(ints, auto_reset=auto_reset, consts=O.MAPPO_CONSTS)
        out = [self.b[e].step(ints[e:e + 1], auto_reset=auto_reset, consts=O.MAPPO_CONSTS) for e in ids]
        return tuple(np.concatenate([o[k] for o in out]) if out else np.zeros(0, dt)
                     for k, dt in enumerate((np.float64, np.float32, bool)))

    def state(self, light):
        """Every env's state (robots, pkgs, t, total_reward) and tracker rows; light: robots only."""
        st = [b.env(i).state() for b, i in map(self._at, range(self.E))]
        s = dict(robots=np.stack([x["robots"] for x in st]))
        if not light:
            s.update(pkgs=np.stack([x["pkgs"] for x in st]), t=np.array([x["t"] for x in st], np.int32),
                     total_reward=np.array([x["total_reward"] for x in st], np.float64),
                     rows=[b.tracker(i).rows() for b, i in map(self._at, range(self.E))])
        return s

    def obs(self, case):
        dims = (case.T, case.A - 1, MP, MR, MPS)
        if not self.singles:
            return self.b.obs(*dims)
        per = [b.obs(*dims) for b in self.b]
        return {k: np.concatenate([o[k] for o in per]) for k in OBS_KEYS}


def _calls(case):
    """The case's calls before the oracle has run: (step index, env ids or None for the full batch)."""
    E = case.E
    for k in range(n_steps(case)):
        ids = None
        if case.subset and k % 4 == 1:   # E - 1 envs in descending, rotated order; every env is left out in turn
            ids = np.roll([e for e in reversed(range(E)) if e != (k // 4) % E], k // 4).astype(np.int32)
            assert len(ids) < E and not (np.diff(ids) > 0).all()
        yield k, ids


def oracle_trace(case, light=False):
    """The oracle's results of every call of the case: a list of dicts with ids (None: all envs; the
    episode form: mask / mask_after instead), ints [E, A], r, sh, done (rows in the order of ids) and
    the state of all E envs after the call (light: the robots only, no observations)."""
    ints = trainer_ints(case)
    with_obs = case.variant in ("obs", "episode") and not light
    trace = []
    if case.variant != "episode":
        orc = _Oracle(case, singles=case.subset)
        for k, ids in _calls(case):
            if ids is None and case.subset:
                r, sh, dn = orc.step(np.arange(case.E), ints[k], True)
            else:
                r, sh, dn = orc.step(ids, ints[k], True)
            trace.append(dict(ids=ids, ints=ints[k], r=r, sh=sh, done=dn, state=orc.state(light),
                              obs=orc.obs(case) if with_obs else None))
        return trace
    orc = _Oracle(case, singles=True)   # never a reset: stepped only where the mask is set
    mask = np.ones(case.E, bool)
    for k in range(case.T):
        for e, at in EPISODE_CUTS.items():
            if at == k:
                mask[e] = False
        for m in ([np.zeros(case.E, bool)] if k == EPISODE_ZERO_MASK_STEP else []) + [mask.copy()]:
            idx = np.nonzero(m)[0]
            r, sh, dn = (np.zeros(case.E, np.float64), np.zeros(case.E, np.float32), np.zeros(case.E, bool))
            r[idx], sh[idx], dn[idx] = orc.step(idx, ints[k], False)
            trace.append(dict(mask=m, mask_after=m & ~dn, ints=ints[k], r=r, sh=sh, done=dn, state=orc.state(light),
                              obs=orc.obs(case) if with_obs else None))
        mask &= ~trace[-1]["done"]
    return trace


def _picks(trace):
    return any((c["state"]["robots"][:, :, 2] > 0).any() for c in trace)


def _delivers(trace):
    return any((c["r"] > 0.5).any() for c in trace)


def _done_counts(case, trace):
    n = np.zeros(case.E, np.int64)
    for c in trace:
        if c.get("ids") is None:
            n += c["done"]
        else:
            n[c["ids"]] += c["done"]
    return n


@functools.lru_cache(maxsize=None)
def _family_deliveries(variant, tracker):
    """How many cases of one kernel family and tracker mode see a delivery, of how many."""
    fam = [c for c in CASES if c.variant == variant and c.tracker == tracker]
    return sum(_delivers(oracle_trace(c, light=True)) for c in fam), len(fam)


def check_inputs(case, trace):
    """The conditions on the inputs, from the oracle's trace alone."""
    assert _picks(trace), "no robot ever carries a package: the case would pass without a pick-up"
    if case.variant != "episode":
        assert (_done_counts(case, trace) >= 2).all(), "every env must finish two episodes (the reset path)"
    else:
        masks = [c["mask"] for c in trace]   # one call per step up to the all-zero call: its index is its step
        assert masks[0].all() and masks[2].all() and not masks[EPISODE_ZERO_MASK_STEP].any()
        assert all(not masks[at][e] and masks[at - 1][e] for e, at in EPISODE_CUTS.items() if at < EPISODE_ZERO_MASK_STEP)
        assert not trace[-1]["mask_after"].any() and trace[-1]["done"].sum() == case.E - len(EPISODE_CUTS)
        assert len({int(m.sum()) for m in masks}) == len(EPISODE_CUTS) + 2   # E, E-1, 0, E-2, E-3 envs active
    got, of = _family_deliveries(case.variant, case.tracker)
    assert 2 * got >= of, f"only {got} of the {of} {case.variant} / {case.tracker} cases see a delivery"


# ------------------------------------------------------------------ the engine side
def same(got, want, what):
    """Bit-for-bit equality of two arrays (so -0.0 != +0.0), with numpy's report on a mismatch."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        np.testing.assert_array_equal(got, want, err_msg=what)
        raise AssertionError(f"{what}: equal values, different bits")


def snap(env):
    s = env.read_state()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in s.items()}


def check_state(env, want, what):
    """read_state and the tracker rows of every env against the oracle's; returns the snapshot."""
    s = snap(env)
    same(s["robots"], want["robots"], f"{what}: robots")
    same(s["pkgs"], want["pkgs"], f"{what}: packages")
    same(s["t"], want["t"], f"{what}: t")
    same(s["total_reward"], want["total_reward"], f"{what}: total_reward")
    for e in range(env.E):
        same(env.tracker_rows(s, e), want["rows"][e], f"{what}: tracker rows of env {e}")
    return s


def check_out(r, sh, dn, c, what):
    same(r.cpu().numpy(), c["r"], f"{what}: r_env")
    same(sh.cpu().numpy(), c["sh"], f"{what}: r_shaped")
    same(dn.cpu().numpy().astype(bool), c["done"], f"{what}: done")


def _template_args(symbol):
    return symbol[symbol.index("<") + 1:-1].split(", ")


def _acts(case, ints):
    """(format, device tensor) of one call's -- or the whole block's -- actions: trainer ints for the
    stale-tracker entries, the same actions as code bytes for the fresh ones."""
    fmt = "int" if case.tracker == "mappo" else "codes"
    return fmt, torch.from_numpy(ints if fmt == "int" else codes_of(ints)).cuda()


def run_plain(case, env, trace):
    layout = {"plain": "wave", "rows": "rows", "halves": "halves"}[case.variant]
    assert env.step_kernel_name(layout) == case.symbol
    for k, c in enumerate(trace):
        fmt, a = _acts(case, c["ints"])
        r, sh, dn = env.step(a, auto_reset=True, action_format=fmt)
        assert env.last_step_layout() == layout
        check_out(r, sh, dn, c, f"step {k}")
        check_state(env, c["state"], f"step {k}")


def run_fused(case, env, trace):
    st, nch, _, au = _template_args(case.symbol)   # the engine names only the per-step twin: the same rule
    assert env.step_kernel_name("wave") == f"mdl::k_step<{st}, {nch}, false, {au}>"
    fmt, a = _acts(case, np.stack([c["ints"] for c in trace]))
    r, sh, dn = env.step_fused(a, auto_reset=True, action_format=fmt)
    want = {k: np.stack([c[k] for c in trace]) for k in ("r", "sh", "done")}
    check_out(r, sh, dn, want, f"{len(trace)} fused steps")
    check_state(env, trace[-1]["state"], "after the fused steps")


def run_mail(case, env, trace):
    assert _template_args(env.step_kernel_name("wave"))[:2] == _template_args(case.symbol)[:2]
    mb = env.mailbox()
    E = case.E
    for k, c in enumerate(trace):
        codes = codes_of(c["ints"])
        ids = np.arange(E) if c["ids"] is None else c["ids"]
        n = len(ids)
        if c["ids"] is not None:
            mb["ids"][:n] = ids
        mb["codes"][:n] = codes[ids]
        env.mail_step(n, c["ids"] is not None, auto_reset=True)
        what = f"call {k} ({n} envs)"
        same(mb["r_env"][:n].copy(), c["r"], f"{what}: mailbox r_env")
        same(mb["r_shaped"][:n].copy(), c["sh"], f"{what}: mailbox r_shaped")
        same(mb["done"][:n].astype(bool), c["done"], f"{what}: mailbox done")
        s = check_state(env, c["state"], what)
        same(mb["robots"][:n].copy(), s["robots"][ids], f"{what}: mailbox robot rows")
        same(mb["pkgs"][:n].copy(), s["pkgs"][ids], f"{what}: mailbox package rows")
        same(mb["t"][:n].copy(), s["t"][ids], f"{what}: mailbox t")
        same(mb["total_reward"][:n].copy(), s["total_reward"][ids], f"{what}: mailbox total_reward")


def _check_obs_dims(case, env):
    assert (env.obs_T, env.MO, env.MP, env.MR, env.MPs) == (case.T, case.A - 1, MP, MR, MPS)


def run_obs(case, env, trace):
    assert env.step_kernel_name(with_obs=True) == case.symbol
    _check_obs_dims(case, env)
    for k, c in enumerate(trace):
        fmt, a = _acts(case, c["ints"])
        r, sh, dn, obs = env.step_obs(a, auto_reset=True, action_format=fmt)
        check_out(r, sh, dn, c, f"step {k}")
        for key in OBS_KEYS:
            same(obs[key].cpu().numpy(), c["obs"][key], f"step {k}: {key}")
        check_state(env, c["state"], f"step {k}")


def run_episode(case, env, trace):
    assert env.step_kernel_name(with_obs=True) == case.symbol.replace("k_step_episode", "k_step_obs")
    _check_obs_dims(case, env)
    E = case.E
    obs_out = env.obs_buffers()
    out = (torch.zeros(E, dtype=torch.float64, device="cuda"), torch.zeros(E, dtype=torch.float32, device="cuda"),
           torch.zeros(E, dtype=torch.uint8, device="cuda"))
    filled = torch.zeros(E, dtype=torch.uint8, device="cuda")
    sent = np.float32(SENTINEL).view(np.uint32)
    for k, c in enumerate(trace):
        what = f"call {k} (mask {c['mask'].astype(int).tolist()})"
        fmt, a = _acts(case, c["ints"])
        active = torch.from_numpy(c["mask"].astype(np.uint8)).cuda()
        for v in obs_out.values():
            v.fill_(SENTINEL)
        out[0].fill_(float("nan"))
        out[1].fill_(float("nan"))
        out[2].fill_(9)
        filled.fill_(9)
        r, sh, dn, obs = env.step_episode(a, active, action_format=fmt, out=out, filled=filled, obs_out=obs_out)
        check_out(r, sh, dn, c, what)   # the oracle's rows of the inactive envs are +0 / not done
        same(filled.cpu().numpy(), c["mask"].astype(np.uint8), f"{what}: filled")
        same(active.cpu().numpy().astype(bool), c["mask_after"], f"{what}: the mask after the call")
        on, off = np.nonzero(c["mask"])[0], np.nonzero(~c["mask"])[0]
        for key in OBS_KEYS:
            x = obs[key].cpu().numpy()
            same(x[on], c["obs"][key][on], f"{what}: {key} rows of the stepped envs")
            assert (x[off].view(np.uint32) == sent).all(), f"{what}: {key} rows of the inactive envs were written"
        check_state(env, c["state"], what)


RUN = dict(plain=run_plain, rows=run_plain, halves=run_plain, fused=run_fused, mail=run_mail, obs=run_obs,
           episode=run_episode)


@pytest.mark.parametrize("case", CASES, ids=[c.symbol for c in CASES])
def test_step_kernel_vs_oracle(case):
    import marl_gpu
    trace = oracle_trace(case)
    check_inputs(case, trace)
    layout = {"rows": "rows", "halves": "halves"}.get(case.variant, "wave")
    env = marl_gpu.BatchedEnv(grid(case.map), case.E, case.A, case.P, case.T, seed=case.seed, tracker=case.tracker,
                              shaping="mappo", max_packages_obs=MP, step_layout=layout)
    try:
        env.reset()
        RUN[case.variant](case, env, trace)
    finally:
        env.close()
