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

from ._capture import Graphed, capture, eval_mode
from .actions import select_actions_eps_mark, select_actions_eps_mark_dev
from .replay import JointReplay


class QmixCycleCollector(Graphed):
    """``QMixTrainer.collect_and_train_cycle``'s environment side (qmix/trainer.py:324-403) on the
    device.

    env: a ``BatchedEnv`` whose envs share one map shape, tracker="fresh" or a stale tracker (which
    the lazy reset empties, as the trainer replaces ``persistent_packages`` by ``{}``).
    replay: a ``JointReplay`` with obs_shape (6, H, W) ((6, K, K) with ``ego_radius``) and state_shape
    (7, h, w) on the env's device.
    hidden_dim None: ``agent(obs [E*A, 6, H, W]) -> q [E*A, n_actions]``.  Otherwise the agent is
    recurrent, ``agent(obs, hidden [E*A, hidden_dim]) -> (q, new_hidden)``; the reference's ``None``
    hidden state is the zero row here.

    ``done`` is the public device mask (uint8 [E]) of the envs whose episode has ended: the next
    ``step`` resets them.  A caller may set a byte to cut an episode short.

    ``begin()`` is the trainer's constructor; ``step(agent, epsilon)`` one iteration of the cycle's
    outer loop for all envs (the caller trains between steps); ``cycle`` runs several.  Env state,
    ``done`` and the hidden state carry over between steps and cycles, as in the reference.  Nothing
    in ``step`` synchronises with the host.

    ego_radius=R (1..15): the agents' observations are each robot's ``K x K`` window (K = 2R + 1) of its
    convert_state tensor (``BatchedEnv.build_obs_alt_ego``, float32) instead of the whole map: the
    replay must hold (6, K, K) observations, ``obs`` is [2, E, A, 6, K, K] and the agent receives
    [E*A, 6, K, K].  The state keeps its (7, h, w); everything but the observations is the full-map
    form's.
    """

    def __init__(self, env, replay: JointReplay, seed: int = 0, hidden_dim: int | None = None,
                 ego_radius: int | None = None):
        self.env, self.replay = env, replay
        self.seed = int(seed)
        self.ego_radius = None if ego_radius is None else env._ego_radius(ego_radius)
        self._init_graphs(env.device)
        E, A = env.E, env.A
        H, W = env.single_map_shape("QmixCycleCollector")
        if self.ego_radius is not None:
            H = W = 2 * self.ego_radius + 1
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
        self._observe(self.obs[0], self.state[0])
        if self.hidden is not None:
            self.hidden.zero_()
        self.done.zero_()

    def _observe(self, o, s):
        """Every env's observations (whole maps, or the windows) and state into o, s."""
        env = self.env
        if self.ego_radius is None:
            env.build_obs_alt(out={"idq_obs": o, "qmix_state": s}, state_shape=self.state_shape)
        else:
            env.build_obs_alt(out={"qmix_state": s}, state_shape=self.state_shape, which=("qmix_state",))
            env.build_obs_alt_ego(self.ego_radius, out=o)

    def _step(self, agent, epsilon, dev_args, k, completed, completed_return):
        env = self.env
        E, A = env.E, env.A
        c = self.cur
        o, o2, s, s2 = self.obs[c], self.obs[1 - c], self.state[c], self.state[1 - c]
        if self.ego_radius is None:
            env.cycle_begin(self.done, out={"idq_obs": o, "qmix_state": s}, completed=completed,
                            completed_return=completed_return, completed_steps=self.completed_steps,
                            state_shape=self.state_shape)
        else:   # the reset envs' state from the lazy reset's launch, their windows under its `completed`
            env.cycle_begin(self.done, out={"qmix_state": s}, completed=completed,
                            completed_return=completed_return, completed_steps=self.completed_steps,
                            state_shape=self.state_shape)
            env.build_obs_alt_ego(self.ego_radius, rows=completed, out=o)
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
        self._observe(o2, s2)
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
        addresses) and step count replay it -- bit-identical to eager calls, in any interleaving (the
        graph rule, ``_capture``; epsilon lives on the device, as the replay cursor does).  A cycle
        of an odd number of steps ends on the other observation slot, which has a graph of its own."""
        n = int(n_steps)
        if n < 1:
            raise ValueError("cycle: n_steps must be >= 1")
        dev = self.env.device
        if self.cycle_completed is None or self.cycle_completed.shape[0] != n:
            self.cycle_completed = torch.zeros((n, self.env.E), dtype=torch.uint8, device=dev)
            self.cycle_completed_return = torch.zeros((n, self.env.E), dtype=torch.float64, device=dev)
            self._graphs.clear()      # they write the old buffers
        with eval_mode(agent):
            if not graph:
                self._run(agent, float(epsilon), False, n)
                return self.cycle_completed, self.cycle_completed_return
            if not self._graphs.matches((agent,), (n,)):
                self._run(agent, float(epsilon), False, n)   # this call's steps, and the warm-up
                self._capture(agent, n)
                return self.cycle_completed, self.cycle_completed_return
            g = self._graphs.lookup((agent,), (n,), self.cur) or self._capture(agent, n)
            self._eps_dev.fill_(float(epsilon))
            self._replay((g,), n)
            self.cur = (self.cur + n) & 1
            return self.cycle_completed, self.cycle_completed_return

    def _capture(self, agent, n):
        """Capture n steps that start on the current slot (the capture itself runs nothing)."""
        off0, cur0 = self.offset, self.cur
        g, _ = capture(self.env.device, lambda: self._run(agent, 0.0, True, n))
        self.offset, self.cur = off0, cur0
        self._graphs.store((agent,), (n,), cur0, g, n)
        return g

    def _run(self, agent, epsilon, dev_args, n):
        for k in range(n):
            self._step(agent, epsilon, dev_args, k, self.cycle_completed[k], self.cycle_completed_return[k])
