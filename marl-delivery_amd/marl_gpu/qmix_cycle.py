"""Device-resident map-QMIX cycle collection (the lower-case ``qmix/`` trainer's environment side).

Replaces the host side of ``QMixTrainer.collect_and_train_cycle`` (qmix/trainer.py:324-403): the
continuous loop over the envs in which a finished env is reset lazily at the start of the next time
step (its tracker emptied, its agents' hidden state dropped, its episode reward banked), the
per-agent ``convert_state`` / ``select_action`` calls with the recurrent agent's hidden state, the
``Environment.step``, the tracker update, ``convert_global_state_to_tensor`` before and after the
step, and the joint ``ReplayBuffer.add``.  Here one launch does the lazy reset and the observations
of the reset rows (``BatchedEnv.cycle_begin``), the agent's Q-values become actions on the device
(``select_actions_eps_mark``, which also reports the rows that explored), the engine steps every env
and builds the next observations (the stored ``next_obs`` / ``next_state`` of a finished env are
those of its terminal state), and ``JointReplay.add`` appends one joint row per env to a device
ring.  Only the agent network's forward pass and the learner are the caller's.
"""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream_handle
from .qmix_rollout import _q_avail


def select_actions_eps_mark(q: torch.Tensor, epsilon: float, seed: int, offset: int, avail=None, out=None,
                            explored=None):
    """``select_actions_eps`` (the same actions, bit for bit) that also reports which rows explored:
    returns (actions uint8 [N], explored uint8 [N]); explored is 1 where the row's uniform fell
    below epsilon and the row had an available action."""
    q, avail = _q_avail(q, avail)
    N, n_act = q.shape
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=q.device)
    if explored is None:
        explored = torch.empty(N, dtype=torch.uint8, device=q.device)
    check(lib().mdl_select_actions_eps_mark(ptr(q), ptr(avail), N, n_act, float(epsilon), seed & (2**64 - 1),
                                            offset & (2**64 - 1), ptr(out), ptr(explored),
                                            stream_handle(q.device)), "mdl_select_actions_eps_mark")
    return out, explored


def select_actions_eps_mark_dev(q: torch.Tensor, epsilon_dev: torch.Tensor, seed: int, offset_dev: torch.Tensor,
                                offset_add: int, avail=None, out=None, explored=None):
    """``select_actions_eps_mark`` with epsilon (float32 tensor [1]) and the offset base (uint64 bits
    in an int64 tensor [1]) read on the device, so the launch can live in a replayed hipGraph."""
    q, avail = _q_avail(q, avail)
    N, n_act = q.shape
    if epsilon_dev.dtype != torch.float32 or offset_dev.dtype != torch.int64:
        raise TypeError("epsilon_dev must be float32 and offset_dev int64 (uint64 bits)")
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=q.device)
    if explored is None:
        explored = torch.empty(N, dtype=torch.uint8, device=q.device)
    check(lib().mdl_select_actions_eps_mark_dev(ptr(q), ptr(avail), N, n_act, ptr(epsilon_dev), seed & (2**64 - 1),
                                                ptr(offset_dev), offset_add & (2**64 - 1), ptr(out), ptr(explored),
                                                stream_handle(q.device)), "mdl_select_actions_eps_mark_dev")
    return out, explored


def _shape(s):
    return (int(s),) if isinstance(s, int) else tuple(int(x) for x in s)


class JointReplay:
    """The ``qmix/`` trainer's joint ``ReplayBuffer`` (qmix/networks.py:155-239) as a device ring,
    its tensors named and shaped as the reference's arrays: states / next_states float32
    [capacity, *state_shape], observations / next_observations float32 [capacity, A, *obs_shape],
    actions int64 [capacity, A], total_reward float32 [capacity, 1], dones uint8 [capacity, 1], and
    the cursor (ptr, size) as an int64 tensor [2] on the device, advanced by ``add`` without a host
    round trip."""

    def __init__(self, capacity: int, n_agents: int, obs_shape, state_shape, device="cuda"):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("JointReplay: capacity must be >= 1")
        self.n_agents = int(n_agents)
        if self.n_agents < 1:
            raise ValueError("JointReplay: n_agents must be >= 1")
        self.obs_shape, self.state_shape = _shape(obs_shape), _shape(state_shape)
        self.device = torch.device(device)
        self.obs_floats = self.state_floats = 1
        for s in self.obs_shape:
            self.obs_floats *= s
        for s in self.state_shape:
            self.state_floats *= s
        f = dict(dtype=torch.float32, device=self.device)
        cap, A = self.capacity, self.n_agents
        self.states = torch.zeros((cap,) + self.state_shape, **f)
        self.next_states = torch.zeros((cap,) + self.state_shape, **f)
        self.observations = torch.zeros((cap, A) + self.obs_shape, **f)
        self.next_observations = torch.zeros((cap, A) + self.obs_shape, **f)
        self.actions = torch.zeros((cap, A), dtype=torch.int64, device=self.device)
        self.total_reward = torch.zeros((cap, 1), **f)
        self.dones = torch.zeros((cap, 1), dtype=torch.uint8, device=self.device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)

    def add(self, state, next_state, obs, next_obs, actions, reward, done):
        """One step's ``buffer.add`` calls (qmix/trainer.py:380-388), one joint row per env in env
        order: state / next_state float32 [E, *state_shape], obs / next_obs float32
        [E, A, *obs_shape], actions uint8 [E, A], reward float64 [E] (stored rounded once to
        float32), done uint8 [E], all contiguous on the ring's device.  Two launches, no
        synchronisation.  A step with more envs than ``capacity`` leaves its last ``capacity`` rows,
        as the sequential adds do."""
        E, A = actions.shape
        if A != self.n_agents:
            raise ValueError(f"JointReplay.add: actions has {A} agents, the ring {self.n_agents}")
        want = dict(state=(state, torch.float32, E * self.state_floats),
                    next_state=(next_state, torch.float32, E * self.state_floats),
                    obs=(obs, torch.float32, E * A * self.obs_floats),
                    next_obs=(next_obs, torch.float32, E * A * self.obs_floats),
                    actions=(actions, torch.uint8, E * A), reward=(reward, torch.float64, E),
                    done=(done, torch.uint8, E))
        for name, (t, dt, n) in want.items():
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.device != self.cursor.device:
                raise TypeError(f"JointReplay.add: {name} must be a contiguous {dt} tensor on {self.cursor.device}")
            if t.numel() != n:
                raise ValueError(f"JointReplay.add: {name} holds {t.numel()} entries, needs {n}")
        check(lib().mdl_replay_append_joint(E, A, self.state_floats, self.obs_floats, ptr(state), ptr(next_state),
                                            ptr(obs), ptr(next_obs), ptr(actions), ptr(reward), ptr(done),
                                            self.capacity, ptr(self.cursor), ptr(self.states), ptr(self.next_states),
                                            ptr(self.observations), ptr(self.next_observations), ptr(self.actions),
                                            ptr(self.total_reward), ptr(self.dones),
                                            stream_handle(self.cursor.device)), "mdl_replay_append_joint")

    def position(self):
        """(ptr, size) read from the device: one 16-byte copy and a synchronisation."""
        p, s = self.cursor.tolist()
        return int(p), int(s)

    def __len__(self):
        """The number of stored rows.  Reads the device cursor (``position``): it synchronises."""
        return self.position()[1]

    def can_sample(self, batch_size: int) -> bool:
        return len(self) >= int(batch_size)

    def sample(self, batch_size: int, generator=None):
        """``ReplayBuffer.sample`` (qmix/networks.py:200-235): ``batch_size`` distinct stored rows as
        the reference's tuple in the reference's order, (states, next_states, obs, next_obs,
        actions int64, total_rewards float32 [B, 1], dones float32 [B, 1]); with fewer than
        ``batch_size`` rows stored, all of them in ring order; an empty ring gives empty tensors.
        Reads the device cursor (a synchronisation): sampling sits on the learner's side of the
        loop.  The draw is torch's ``randperm`` (``generator``), not numpy's global stream."""
        size = len(self)
        if size < int(batch_size):
            idx = torch.arange(size, device=self.device)
        else:
            gdev = generator.device if generator is not None else torch.device("cpu")
            idx = torch.randperm(size, generator=generator, device=gdev)[:int(batch_size)].to(self.device)
        return (self.states[idx], self.next_states[idx], self.observations[idx], self.next_observations[idx],
                self.actions[idx], self.total_reward[idx], self.dones[idx].float())


class QmixCycleCollector:
    """``QMixTrainer.collect_and_train_cycle``'s environment side (qmix/trainer.py:324-403) on the
    device.

    env: a ``BatchedEnv`` whose envs share one map shape, tracker="fresh" or a stale tracker (which
    the lazy reset empties, as the trainer replaces ``persistent_packages`` by ``{}``).
    replay: a ``JointReplay`` with obs_shape (6, H, W) and state_shape (7, h, w) on the env's device.
    hidden_dim None: ``agent(obs [E*A, 6, H, W]) -> q [E*A, n_actions]``.  Otherwise the agent is
    recurrent, ``agent(obs, hidden [E*A, hidden_dim]) -> (q, new_hidden)``; the reference's ``None``
    hidden state is the zero row here.

    ``done`` is the public device mask (uint8 [E]) of the envs whose episode has ended: the next
    ``step`` resets them.  A caller may set a byte to cut an episode short.

    ``begin()`` is the trainer's constructor; ``step(agent, epsilon)`` one iteration of the cycle's
    outer loop for all envs (the caller trains between steps); ``cycle`` runs several.  Env state,
    ``done`` and the hidden state carry over between steps and cycles, as in the reference.  Nothing
    in ``step`` synchronises with the host.
    """

    def __init__(self, env, replay: JointReplay, seed: int = 0, hidden_dim: int | None = None):
        self.env, self.replay = env, replay
        self.seed = int(seed)
        self.offset = 0
        E, A = env.E, env.A
        if env._shape_run_end[0] < E:
            raise ValueError("QmixCycleCollector: the engine's envs mix map shapes (build one engine per map shape)")
        H, W = env.grids[int(env.env_map[0])].shape
        ss = replay.state_shape
        if replay.obs_shape != (6, H, W) or len(ss) != 3 or ss[0] != 7 or replay.n_agents != A \
                or replay.cursor.device != env.device:
            raise ValueError(f"QmixCycleCollector: replay must hold {A} agents' (6, {H}, {W}) observations and "
                             f"(7, h, w) states on {env.device}")
        self.state_shape = ss
        dev = env.device
        b = dict(dtype=torch.uint8, device=dev)
        self.obs = torch.zeros((2, E, A, 6, H, W), dtype=torch.float32, device=dev)
        self.state = torch.zeros((2, E) + ss, dtype=torch.float32, device=dev)
        self.cur = 0                                  # the slot holding the current observations and state
        self.hidden_dim = None if hidden_dim is None else int(hidden_dim)
        self.hidden = None if hidden_dim is None else torch.zeros((E * A, self.hidden_dim), dtype=torch.float32,
                                                                  device=dev)
        self.u = torch.zeros((E, A), **b)
        self.explored = torch.zeros(E * A, **b)
        self.r_env = torch.zeros(E, dtype=torch.float64, device=dev)
        self.r_shaped = torch.zeros(E, dtype=torch.float32, device=dev)
        self.done = torch.zeros(E, **b)
        self.completed = torch.zeros(E, **b)
        self.completed_return = torch.zeros(E, dtype=torch.float64, device=dev)
        self.completed_steps = torch.zeros(E, dtype=torch.int32, device=dev)
        self.cycle_completed = None          # [n_steps, E] uint8, written by cycle
        self.cycle_completed_return = None   # [n_steps, E] float64
        self._graphs = {}             # starting slot -> hipGraph of one whole cycle (cycle(graph=True))
        self._graph_key = None        # (agent, parameter addresses, steps) the graphs were captured with
        self._off_dev = torch.zeros(1, dtype=torch.int64, device=dev)   # selection offset base (uint64 bits)
        self._eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def begin(self):
        """The trainer's constructor (qmix/trainer.py:146-156): a stale tracker is cleared, every env
        is reset, the observations and the state go into slot 0, the hidden state is zeroed and
        ``done`` is 0."""
        env = self.env
        if env.tracker != "fresh":
            env.clear_tracker()   # before the reset, whose tracker update then inserts the t = 0 packages
        env.reset()
        self.cur = 0
        env.build_obs_alt(out={"idq_obs": self.obs[0], "qmix_state": self.state[0]}, state_shape=self.state_shape)
        if self.hidden is not None:
            self.hidden.zero_()
        self.done.zero_()

    def _step(self, agent, epsilon, dev_args, k, completed, completed_return):
        env = self.env
        E, A = env.E, env.A
        c = self.cur
        o, o2, s, s2 = self.obs[c], self.obs[1 - c], self.state[c], self.state[1 - c]
        env.cycle_begin(self.done, out={"idq_obs": o, "qmix_state": s}, completed=completed,
                        completed_return=completed_return, completed_steps=self.completed_steps,
                        state_shape=self.state_shape)
        flat = o.reshape(E * A, *o.shape[2:])
        if self.hidden is None:
            q = agent(flat)
        else:
            # a reset env's agents start from no hidden state (qmix/trainer.py:341)
            self.hidden.view(E, A, -1).masked_fill_(completed.bool().view(E, 1, 1), 0.0)
            q, new_hidden = agent(flat, self.hidden)
        if dev_args:
            select_actions_eps_mark_dev(q, self._eps_dev, self.seed, self._off_dev, k, out=self.u.view(-1),
                                        explored=self.explored)
        else:
            select_actions_eps_mark(q, epsilon, self.seed, self.offset, out=self.u.view(-1), explored=self.explored)
        self.offset += 1
        if self.hidden is not None:
            # an exploring agent never ran its network: its hidden state stays (qmix/trainer.py:251-260)
            self.hidden.copy_(torch.where(self.explored.bool().unsqueeze(1), self.hidden, new_hidden))
        env.step(self.u, auto_reset=False, out=(self.r_env, self.r_shaped, self.done))
        env.build_obs_alt(out={"idq_obs": o2, "qmix_state": s2}, state_shape=self.state_shape)
        self.replay.add(s, s2, o, o2, self.u, self.r_env, self.done)
        self.cur = 1 - c

    @torch.no_grad()
    def step(self, agent, epsilon: float):
        """One time step of every env: the lazy reset of the envs ``done`` marks, forward,
        epsilon-greedy selection (the library's random stream), the step, the next observations,
        the replay append.  Returns (r_env float64 [E], completed uint8 [E], completed_return
        float64 [E]): the collector's own device tensors, overwritten by the next step;
        ``completed_steps`` holds the finished episodes' lengths."""
        self._step(agent, float(epsilon), False, 0, self.completed, self.completed_return)
        return self.r_env, self.completed, self.completed_return

    @torch.no_grad()
    def cycle(self, agent, epsilon: float, n_steps: int, graph: bool = False):
        """``n_steps`` steps (it does not call ``begin``).  Returns (completed uint8 [n_steps, E],
        completed_return float64 [n_steps, E]), the collector's own tensors: row k holds step k's
        lazily reset envs and their episodes' returns, so the returns in (step, env) order are the
        reference's ``cycle_completed_episode_rewards``.  The forward passes run with the agent in
        eval mode (if it has ``eval`` / ``train``); its mode is restored afterwards.

        graph=True: the first call runs eagerly and captures the whole cycle as one hipGraph; later
        calls with the same agent (the very same module, its parameters still at the captured
        addresses) and step count replay it -- bit-identical to eager calls (epsilon and the
        selection's offset base live on the device, as the replay cursor does).  A cycle of an odd
        number of steps ends on the other observation slot, which has a graph of its own."""
        n = int(n_steps)
        if n < 1:
            raise ValueError("cycle: n_steps must be >= 1")
        dev = self.env.device
        if self.cycle_completed is None or self.cycle_completed.shape[0] != n:
            self.cycle_completed = torch.zeros((n, self.env.E), dtype=torch.uint8, device=dev)
            self.cycle_completed_return = torch.zeros((n, self.env.E), dtype=torch.float64, device=dev)
            self._graphs, self._graph_key = {}, None
        was_training = bool(getattr(agent, "training", False))
        if hasattr(agent, "eval"):
            agent.eval()
        try:
            if not graph:
                self._run(agent, float(epsilon), False, n)
                return self.cycle_completed, self.cycle_completed_return
            ptrs = tuple(q.data_ptr() for q in agent.parameters()) if hasattr(agent, "parameters") else ()
            k0 = self._graph_key
            if k0 is None or k0[0] is not agent or k0[1] != ptrs or k0[2] != n:
                self._graphs, self._graph_key = {}, (agent, ptrs, n)
                self._run(agent, float(epsilon), False, n)   # this call's steps, and the warm-up
                self._capture(agent, n)
                return self.cycle_completed, self.cycle_completed_return
            if self.cur not in self._graphs:
                self._capture(agent, n)
            self._eps_dev.fill_(float(epsilon))
            self._off_dev.fill_(self.offset)
            self._graphs[self.cur].replay()
            self.offset += n
            self.cur = (self.cur + n) & 1
            return self.cycle_completed, self.cycle_completed_return
        finally:
            if was_training and hasattr(agent, "train"):
                agent.train()

    def _capture(self, agent, n):
        """Capture n steps that start on the current slot (the capture itself runs nothing)."""
        dev = self.env.device
        torch.cuda.synchronize(dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        off0, cur0 = self.offset, self.cur
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._run(agent, 0.0, True, n)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        self.offset, self.cur = off0, cur0
        self._graphs[cur0] = g

    def _run(self, agent, epsilon, dev_args, n):
        for k in range(n):
            self._step(agent, epsilon, dev_args, k, self.cycle_completed[k], self.cycle_completed_return[k])
