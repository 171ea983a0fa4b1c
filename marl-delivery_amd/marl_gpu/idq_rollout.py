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

from ._capture import Graphed, capture, eval_mode
from ._lib import check, lib, ptr, stream_handle
from .actions import ACTION_DIM, select_actions_eps, select_actions_eps_dev  # noqa: F401
from .replay import TransitionReplay


class IdqCollector(Graphed):
    """``DQNTrainer.run_episode``'s environment side (IDQ/trainer.py:233-324) on the device.

    env: a ``BatchedEnv`` with tracker="fresh", or a stale tracker, which ``begin`` clears before
    the reset: the trainer starts every episode with empty ``persistent_packages`` and fills them
    from the reset state (IDQ/trainer.py:235-239), which is the reset's own tracker update on an
    empty tracker.  (Cleared after the reset, the packages that start at t = 0 would never be
    inserted: the update inserts a package at its start time only.)
    replay: a ``TransitionReplay`` with obs_shape (6, H, W) on the env's device ((6, K, K) with
    ``ego_radius``).
    agent(obs [E*A, 6, H, W]) -> q [E*A, n_actions], as the reference's ``AgentNetwork``.
    ops_are_ints=False reproduces the trainer, which hands reward_shaping string ops (only the
    stay penalty fires); True gives reward_shaping the integer ops its branches test for.

    ``begin()`` then ``step(agent, epsilon)`` per time step is the reference's train-every-step
    loop (the caller trains between steps); ``collect`` runs a whole episode for
    collect-then-train.  Nothing in ``step`` synchronises with the host.

    One deviation from the reference: its plain ``VectorizedEnv`` keeps stepping finished envs
    with stay actions and ignores the results; here they are not stepped.  Nothing the trainer
    consumes differs (the agent still runs on their stale observation rows: forward time only).

    ego_radius=R (1..15): the observations are each robot's ``K x K`` window (K = 2R + 1) of its
    convert_state tensor (``BatchedEnv.build_obs_alt_ego``, float32) instead of the whole map: the
    replay must hold (6, K, K) observations, ``obs`` is [2, E, A, 6, K, K] and the agent receives
    [E*A, 6, K, K].  Rewards, actions and the ring's other columns are those of the full-map form.
    """

    def __init__(self, env, replay: TransitionReplay, seed: int = 0, ops_are_ints: bool = False,
                 ego_radius: int | None = None):
        self.env, self.replay = env, replay
        self.seed = int(seed)
        self.ops_are_ints = bool(ops_are_ints)
        self.ego_radius = None if ego_radius is None else env._ego_radius(ego_radius)
        self._init_graphs(env.device)
        E, A = env.E, env.A
        H, W = env.single_map_shape("IdqCollector")
        if self.ego_radius is not None:
            H = W = 2 * self.ego_radius + 1
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
        self._eps_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def begin(self):
        """Reset every env and build the first observations (slot 0) and the pre-record."""
        env = self.env
        if env.tracker != "fresh":
            env.clear_tracker()   # before the reset, whose tracker update then inserts the t = 0 packages
        env.reset()
        self.active.fill_(1)
        self.cur = 0
        if self.ego_radius is None:
            env.alt_transition(None, self.pre, out={"idq_obs": self.obs[0]})
        else:
            env.alt_transition(None, self.pre, which=())
            env.build_obs_alt_ego(self.ego_radius, out=self.obs[0])

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
        if self.ego_radius is None:
            env.alt_transition(self.u, self.pre, row_mask=self.filled, ops_are_ints=self.ops_are_ints,
                               out={"idq_obs": o2}, r_out=self.r_idq)
        else:
            env.alt_transition(self.u, self.pre, row_mask=self.filled, ops_are_ints=self.ops_are_ints, which=(),
                               r_out=self.r_idq)
            env.build_obs_alt_ego(self.ego_radius, rows=self.filled, out=o2)
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
        captured addresses) and step count replay it -- bit-identical to eager calls, in any
        interleaving (the graph rule, ``_capture``; epsilon lives on the device, as the replay
        cursor does)."""
        n = self.env.T if max_steps is None else min(int(max_steps), self.env.T)
        with eval_mode(agent):
            if not graph:
                return self._run(agent, float(epsilon), False, n)
            g = self._graphs.lookup((agent,), (n,))
            if g is not None:
                self._eps_dev.fill_(float(epsilon))
                self._replay((g,), n)
                self.cur = n & 1
                return self.episode_return
            out = self._run(agent, float(epsilon), False, n)   # this call's episodes, and the warm-up
            off0, cur0 = self.offset, self.cur
            g, _ = capture(self.env.device, lambda: self._run(agent, 0.0, True, n))
            self.offset, self.cur = off0, cur0   # capture ran nothing
            self._graphs.store((agent,), (n,), None, g, n)
            return out

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
