"""Device-resident IDQ transition collection (the counterpart of ``qmix_rollout.py`` for IDQ).

Replaces the host side of ``DQNTrainer.run_episode`` (IDQ/trainer.py:233-324): the per-env,
per-agent ``convert_state`` / ``select_action`` loop, the ``VectorizedEnv.step``, the per-agent
``reward_shaping`` with the tracker copied before the step, the tracker update and the
per-transition ``buffer.add`` calls.  Here the agent's Q-values become actions on the device
(``select_actions_eps``), the engine steps the envs whose episode still runs
(``BatchedEnv.step_episode``), one more launch turns the step into IDQ's per-agent rewards and
next observations (``BatchedEnv.alt_transition``), and ``TransitionReplay.add`` appends one row
per agent of every stepped env to a device ring, the running-env mask never leaving the device.
Only the agent network's forward pass and the learner are the caller's.
"""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream_handle
from .qmix_rollout import ACTION_DIM, select_actions_eps, select_actions_eps_dev  # noqa: F401


class TransitionReplay:
    """The reference's per-transition ``ReplayBuffer`` (IDQ/networks.py:46-104) as a device ring:
    observations / next_observations float32 [capacity, *obs_shape], actions int64, rewards
    float32, dones uint8 [capacity], and the cursor (ptr, size) as an int64 tensor [2] on the
    device, advanced by ``add`` without a host round trip."""

    def __init__(self, capacity: int, obs_shape, device="cuda"):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("TransitionReplay: capacity must be >= 1")
        self.obs_shape = (int(obs_shape),) if isinstance(obs_shape, int) else tuple(int(s) for s in obs_shape)
        self.device = torch.device(device)
        self.row_floats = 1
        for s in self.obs_shape:
            self.row_floats *= s
        f = dict(dtype=torch.float32, device=self.device)
        self.observations = torch.zeros((self.capacity,) + self.obs_shape, **f)
        self.next_observations = torch.zeros((self.capacity,) + self.obs_shape, **f)
        self.actions = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self.rewards = torch.zeros(self.capacity, **f)
        self.dones = torch.zeros(self.capacity, dtype=torch.uint8, device=self.device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._rank = None   # int32 [E + 3], mdl_replay_append's scratch

    def add(self, filled, obs, actions, reward, next_obs, done):
        """One step's ``buffer.add`` calls (IDQ/trainer.py:304-311): for every env with
        ``filled[e] != 0`` in env order and every agent in order, the row (obs[e, a],
        actions[e, a], reward[e, a], next_obs[e, a], done[e]).  filled / done uint8 [E], obs /
        next_obs float32 [E, A, *obs_shape], actions uint8 [E, A], reward float64 [E, A] (stored
        rounded once to float32), all contiguous on the ring's device.  Two launches, no
        synchronisation.  A step with more rows than ``capacity`` leaves its last ``capacity``
        rows, as the sequential adds do."""
        E, A = actions.shape
        want = dict(filled=(filled, torch.uint8, E), done=(done, torch.uint8, E), actions=(actions, torch.uint8, E * A),
                    reward=(reward, torch.float64, E * A), obs=(obs, torch.float32, E * A * self.row_floats),
                    next_obs=(next_obs, torch.float32, E * A * self.row_floats))
        for name, (t, dt, n) in want.items():
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.device != self.cursor.device:
                raise TypeError(f"TransitionReplay.add: {name} must be a contiguous {dt} tensor on {self.cursor.device}")
            if t.numel() != n:
                raise ValueError(f"TransitionReplay.add: {name} holds {t.numel()} entries, needs {n}")
        if self._rank is None or self._rank.numel() < E + 3:
            self._rank = torch.zeros(E + 3, dtype=torch.int32, device=self.cursor.device)
        check(lib().mdl_replay_append(ptr(filled), E, A, self.row_floats, ptr(obs), ptr(next_obs), ptr(actions),
                                      ptr(reward), ptr(done), self.capacity, ptr(self.cursor), ptr(self.observations),
                                      ptr(self.next_observations), ptr(self.actions), ptr(self.rewards),
                                      ptr(self.dones), ptr(self._rank), stream_handle(self.cursor.device)),
              "mdl_replay_append")

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
        """``ReplayBuffer.sample`` (IDQ/networks.py:81-104): ``batch_size`` distinct stored rows as
        (obs float32, actions int64, rewards float32, next_obs float32, dones float32); with
        fewer than ``batch_size`` rows stored, all of them in ring order.  Reads the device cursor
        (one 16-byte copy and a synchronisation): sampling sits on the learner's side of the
        loop.  The draw is torch's ``randperm`` (``generator``), not numpy's global stream."""
        size = len(self)
        if size < int(batch_size):
            idx = torch.arange(size, device=self.device)
        else:
            gdev = generator.device if generator is not None else torch.device("cpu")
            idx = torch.randperm(size, generator=generator, device=gdev)[:int(batch_size)].to(self.device)
        return (self.observations[idx], self.actions[idx], self.rewards[idx], self.next_observations[idx],
                self.dones[idx].float())


class IdqCollector:
    """``DQNTrainer.run_episode``'s environment side (IDQ/trainer.py:233-324) on the device.

    env: a ``BatchedEnv`` with tracker="fresh", or a stale tracker, which ``begin`` clears before
    the reset: the trainer starts every episode with empty ``persistent_packages`` and fills them
    from the reset state (IDQ/trainer.py:235-239), which is the reset's own tracker update on an
    empty tracker.  (Cleared after the reset, the packages that start at t = 0 would never be
    inserted: the update inserts a package at its start time only.)
    replay: a ``TransitionReplay`` with obs_shape (6, H, W) on the env's device.
    agent(obs [E*A, 6, H, W]) -> q [E*A, n_actions], as the reference's ``AgentNetwork``.
    ops_are_ints=False reproduces the trainer, which hands reward_shaping string ops (only the
    stay penalty fires); True gives reward_shaping the integer ops its branches test for.

    ``begin()`` then ``step(agent, epsilon)`` per time step is the reference's train-every-step
    loop (the caller trains between steps); ``collect`` runs a whole episode for
    collect-then-train.  Nothing in ``step`` synchronises with the host.

    One deviation from the reference: its plain ``VectorizedEnv`` keeps stepping finished envs
    with stay actions and ignores the results; here they are not stepped.  Nothing the trainer
    consumes differs (the agent still runs on their stale observation rows: forward time only).
    """

    def __init__(self, env, replay: TransitionReplay, seed: int = 0, ops_are_ints: bool = False):
        self.env, self.replay = env, replay
        self.seed = int(seed)
        self.ops_are_ints = bool(ops_are_ints)
        self.offset = 0
        E, A = env.E, env.A
        if env._shape_run_end[0] < E:
            raise ValueError("IdqCollector: the engine's envs mix map shapes (build one engine per map shape)")
        H, W = env.grids[int(env.env_map[0])].shape
        if replay.obs_shape != (6, H, W) or replay.cursor.device != env.device:
            raise ValueError(f"IdqCollector: replay must hold (6, {H}, {W}) observations on {env.device}")
        dev = env.device
        b = dict(dtype=torch.uint8, device=dev)
        self.obs = torch.zeros((2, E, A, 6, H, W), dtype=torch.float32, device=dev)
        self.cur = 0                                  # the slot holding the current observations
        self.pre = env.alt_pre_buffer()
        self.u = torch.zeros((E, A), **b)
        self.r_idq = torch.zeros((E, A), dtype=torch.float64, device=dev)
        self.r_env = torch.zeros(E, dtype=torch.float64, device=dev)
        self.r_shaped = torch.zeros(E, dtype=torch.float32, device=dev)
        self.done = torch.zeros(E, **b)
        self.filled = torch.zeros(E, **b)
        self.active = torch.zeros(E, **b)
        self.episode_return = torch.zeros(E, dtype=torch.float64, device=dev)
        self._graph = None            # hipGraph of one whole collect (collect(graph=True))
        self._graph_key = None        # (agent, parameter addresses, steps) the graph was captured with
        self._off_dev = torch.zeros(1, dtype=torch.int64, device=dev)   # selection offset base (uint64 bits)
        self._eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def begin(self):
        """Reset every env and build the first observations (slot 0) and the pre-record."""
        env = self.env
        if env.tracker != "fresh":
            env.clear_tracker()   # before the reset, whose tracker update then inserts the t = 0 packages
        env.reset()
        self.active.fill_(1)
        self.cur = 0
        env.alt_transition(None, self.pre, out={"idq_obs": self.obs[0]})

    def _step(self, agent, epsilon, dev_args, k):
        env = self.env
        E, A = env.E, env.A
        o, o2 = self.obs[self.cur], self.obs[1 - self.cur]
        q = agent(o.reshape(E * A, *o.shape[2:]))
        if dev_args:
            select_actions_eps_dev(q, self._eps_dev, self.seed, self._off_dev, k, out=self.u.view(-1))
        else:
            select_actions_eps(q, epsilon, self.seed, self.offset, out=self.u.view(-1))
        self.offset += 1
        env.step_episode(self.u, self.active, out=(self.r_env, self.r_shaped, self.done), filled=self.filled,
                         obs_out={}, which=())
        env.alt_transition(self.u, self.pre, row_mask=self.filled, ops_are_ints=self.ops_are_ints,
                           out={"idq_obs": o2}, r_out=self.r_idq)
        self.replay.add(self.filled, o, self.u, self.r_idq, o2, self.done)
        self.cur = 1 - self.cur

    @torch.no_grad()
    def step(self, agent, epsilon: float):
        """One time step of every running env: forward, epsilon-greedy selection (rand < eps ->
        randint(0, 15), else the first argmax: IDQ/trainer.py:185-195, the library's random
        stream), the masked step, rewards and next observations, the replay append.  Returns
        (r_env float64 [E], filled uint8 [E]): the collector's own device tensors, overwritten by
        the next step; the global reward of an env that was not stepped is 0."""
        self._step(agent, float(epsilon), False, 0)
        return self.r_env, self.filled

    @torch.no_grad()
    def collect(self, agent, epsilon: float, max_steps: int | None = None, graph: bool = False):
        """``begin`` plus min(max_steps, env.T) steps (every episode ends within env.T).  Returns
        episode_return (float64 [E], each env's ``total_reward``).  The forward passes run with
        the agent in eval mode (if it has ``eval`` / ``train``); its mode is restored afterwards.

        graph=True: the first call runs eagerly and captures the whole collect as one hipGraph;
        later calls with the same agent (the very same module, its parameters still at the
        captured addresses) and step count replay it -- bit-identical to eager calls (epsilon
        and the selection's offset base live on the device, as the replay cursor does)."""
        n = self.env.T if max_steps is None else min(int(max_steps), self.env.T)
        was_training = bool(getattr(agent, "training", False))
        if hasattr(agent, "eval"):
            agent.eval()
        try:
            if not graph:
                return self._run(agent, float(epsilon), False, n)
            ptrs = tuple(q.data_ptr() for q in agent.parameters()) if hasattr(agent, "parameters") else ()
            k0 = self._graph_key
            if self._graph is not None and k0[0] is agent and k0[1] == ptrs and k0[2] == n:
                self._eps_dev.fill_(float(epsilon))
                self._graph.replay()
                self.offset += n
                self.cur = n & 1
                return self.episode_return
            out = self._run(agent, float(epsilon), False, n)   # this call's episodes, and the warm-up
            self._capture(agent, (agent, ptrs, n), n)
            return out
        finally:
            if was_training and hasattr(agent, "train"):
                agent.train()

    def _capture(self, agent, key, n):
        dev = self.env.device
        torch.cuda.synchronize(dev)
        self._off_dev.fill_(self.offset)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        off0, cur0 = self.offset, self.cur
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._run(agent, 0.0, True, n)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        self.offset, self.cur = off0, cur0   # capture ran nothing
        self._graph, self._graph_key = g, key

    def _run(self, agent, epsilon, dev_args, n):
        env = self.env
        self.begin()
        for k in range(n):
            self._step(agent, epsilon, dev_args, k)
        if dev_args:
            check(lib().mdl_counter_add(ptr(self._off_dev), n, stream_handle(env.device)), "mdl_counter_add")
        check(lib().mdl_read_state(env._h, None, None, None, ptr(self.episode_return), None, None,
                                   stream_handle(env.device)), "mdl_read_state")
        return self.episode_return
