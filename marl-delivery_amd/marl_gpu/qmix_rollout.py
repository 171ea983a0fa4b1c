"""Device-resident QMIX episode collection (the counterpart of ``rollout.py`` for QMIX).

Replaces the host side of ``QMixLearner.collect_data_iteration`` and
``select_actions_epsilon_greedy`` (QMIX/trainer.py:258-528): the per-env Python loop that
featurizes the running envs, the epsilon-greedy choice with its per-row ``torch.randint``
loop, the subset ``vec_env.step``, the tracker update, the per-transition dicts and the
numpy replay buffer.  Here the agent's Q-values are turned into actions on the device
(``select_actions_eps``), the engine steps the envs whose episode still runs and featurizes
them straight into time-major episode buffers (``BatchedEnv.step_episode``: one launch, the
running-env mask lives on the device), and ``EpisodeReplay`` keeps the episodes in a device
ring.  Only the agent network's forward pass is the caller's (a torch module, as in the
reference).
"""
from __future__ import annotations

import torch

from ._capture import Graphed, capture, eval_mode
from ._lib import check, lib, ptr, stream_handle
from .actions import ACTION_DIM, select_actions_eps, select_actions_eps_dev  # noqa: F401
from .replay import EpisodeReplay  # noqa: F401


class QmixCollector(Graphed):
    """``collect_data_iteration`` (QMIX/trainer.py:333-528) on the device: one episode per env.

    env: a ``BatchedEnv`` built like the trainer's (shaping="qmix"; tracker="fresh", or a
    stale tracker, which ``collect`` clears after the reset as QMIX/trainer.py:523-526 does).
    agent(so [E*A, 6, H, W], vo [E*A, Dv], h [E*A, Hd]) -> (q [E*A, n_actions], h' [E*A, Hd]),
    with ``agent.init_hidden()`` -> [1, Hd] as the reference's ``AgentNetwork``.

    Time-major buffers, L = min(episode_limit, env.T):
      so [L+1, E, A, 6, H, W] (with ego_radius: [L+1, E, A, 6, K, K], below), vo [L+1, E, A, Dv],
      gs [L+1, E, 4, H, W], gv [L+1, E, Dg]
      (slot t = the observations before step t, slot t+1 = after it), u uint8 [L, E, A],
      r float32 [L, E] (the fp64 global reward rounded once, as the reference's float32
      buffer does; r64 keeps the fp64 values), r_shaped float32 [L, E], terminated and
      filled uint8 [L, E], hidden [E*A, Hd] (the last hidden states).
    Rows of an env past its episode's end (filled == 0) are not written: they hold whatever
    an earlier collect left there.

    avail=True: the selection takes the valid-action mask of each state (``BatchedEnv.avail_actions``,
    one small launch per step, inside the graph too) instead of the reference's all-ones placeholder
    (QMIX/trainer.py:395-397), and ``batch()`` gains avail uint8 [L+1, E, A, n_actions]: slot t = the
    mask the selection of step t used, slot t+1 = the mask after it (all ones for an env whose episode
    has ended: every slot is written).  ``EpisodeReplay`` stores it and returns it as avail_u /
    avail_u_next.  avail=False (the default): nothing changes.

    ego_radius=R (1..15, K = 2R + 1): the agent sees each robot's K x K window of its actor map
    (``BatchedEnv.build_obs_ego``) instead of the full map: so is [L+1, E, A, 6, K, K] of ``ego_dtype``
    (torch.float32, float16 or bfloat16) and the agent is called with so [E*A, 6, K, K] in that type.
    vo, gs, gv stay float32 and the mixer's state keeps the full map (so the envs still share one map
    shape).  Each step is then two launches: ``step_episode`` writes vo / gs / gv, and
    ``build_obs_ego_masked`` under that step's ``filled`` writes the windows of the envs that were
    stepped -- ``filled``, not ``active``, which is already cleared for an env that finished on this
    step while its terminal observation is still due, as the full-map path writes it.  Rows past an
    episode's end stay unwritten, as in the full-map form.  ego_radius=None (the default): nothing changes.

    canvas=(Hc, Wc), with ego_radius (ValueError without it): the mixer's state is the critic map on that
    fixed canvas (``BatchedEnv.build_obs_canvas``: the map in the top-left corner, off-map cells obstacles),
    gs is [L+1, E, 4, Hc, Wc], and the engine may mix map shapes.  Each step is then three calls:
    ``step_episode(which=())``, ``build_obs_canvas(rows=filled[t])`` for gs / vo / gv and
    ``build_obs_ego_masked(filled[t])`` -- both under ``filled``, for the reason above.  The canvas must
    cover every map.  canvas=None (the default): nothing changes.

    One deviation from the reference: the agent also runs on the finished envs (the
    reference shrinks its batch instead).  Their actions and hidden states are ignored --
    the engine does not step them -- so the finished envs cost forward-pass time only.
    """

    def __init__(self, env, episode_limit: int, seed: int = 0, avail: bool = False, ego_radius: int | None = None,
                 ego_dtype: torch.dtype = torch.float32, canvas=None):
        self.env = env
        if canvas is not None and ego_radius is None:
            raise ValueError("QmixCollector: canvas needs ego_radius (the agent's full map has no shape "
                             "common to several maps)")
        self.canvas = None if canvas is None else env._canvas(canvas)
        self.L = L = min(int(episode_limit), env.T)
        if L < 1:
            raise ValueError("QmixCollector: episode_limit must be >= 1")
        self.seed = int(seed)
        self._init_graphs(env.device)
        E, A = env.E, env.A
        H, W = env.single_map_shape("QmixCollector") if self.canvas is None else self.canvas
        dev = env.device
        f = dict(dtype=torch.float32, device=dev)
        b = dict(dtype=torch.uint8, device=dev)
        self.ego_radius = None if ego_radius is None else env._ego_radius(ego_radius)
        self.ego_dtype = ego_dtype
        if self.ego_radius is None:
            self.so = torch.zeros((L + 1, E, A, 6, H, W), **f)
        else:
            K = 2 * self.ego_radius + 1
            env.ego_buffers(self.ego_radius, 0, ego_dtype)   # raises on a dtype the builder does not write
            self.so = torch.zeros((L + 1, E, A, 6, K, K), dtype=ego_dtype, device=dev)
        self.vo = torch.zeros((L + 1, E, A, env.actor_vec_dim), **f)
        self.gs = torch.zeros((L + 1, E, 4, H, W), **f)
        self.gv = torch.zeros((L + 1, E, env.critic_vec_dim), **f)
        self.u = torch.zeros((L, E, A), **b)
        self.r = torch.zeros((L, E), **f)
        self.r64 = torch.zeros((L, E), dtype=torch.float64, device=dev)
        self.r_shaped = torch.zeros((L, E), **f)
        self.terminated = torch.zeros((L, E), **b)
        self.filled = torch.zeros((L, E), **b)
        self.active = torch.zeros(E, **b)
        self.hidden = None            # [E*A, Hd], allocated by the first collect
        self.episode_return = torch.zeros(E, dtype=torch.float64, device=dev)
        self.episode_length = torch.zeros(E, dtype=torch.int64, device=dev)
        self._eps_dev = torch.zeros(1, **f)
        self.avail = torch.ones((L + 1, E, A, ACTION_DIM), **b) if avail else None

    def _slot(self, k):
        if self.ego_radius is not None:   # so[k] holds windows: build_obs_ego's, not the builders'
            return dict(actor_vec=self.vo[k], critic_map=self.gs[k], critic_vec=self.gv[k])
        return dict(actor_map=self.so[k], actor_vec=self.vo[k], critic_map=self.gs[k], critic_vec=self.gv[k])

    def batch(self):
        """The buffers of the last collect (the collector's own tensors, not copies)."""
        out = dict(so=self.so, vo=self.vo, gs=self.gs, gv=self.gv, u=self.u, r=self.r, r64=self.r64,
                   r_shaped=self.r_shaped, terminated=self.terminated, filled=self.filled, hidden=self.hidden,
                   episode_return=self.episode_return, episode_length=self.episode_length)
        if self.avail is not None:
            out["avail"] = self.avail
        return out

    @torch.no_grad()
    def collect(self, agent, epsilon: float, graph: bool = False):
        """One episode of at most L steps in every env, from a fresh reset.  Returns ``batch()``:
        the buffers plus episode_return (fp64 [E], each env's ``total_reward``) and
        episode_length (int64 [E], ``filled.sum(0)``).  The forward passes run with the agent
        in eval mode (if it has ``eval`` / ``train``) and its mode is restored afterwards, as
        QMIX/trainer.py:287-289 does.  Nothing inside the loop synchronises with the host.

        graph=True: the first call runs eagerly and captures the whole collect (reset,
        forwards, selection, steps, observations) as one hipGraph; later calls with the same
        agent replay it -- bit-identical to eager calls, in any interleaving (the graph rule,
        ``_capture``; epsilon lives on the device).  The returned tensors are the graph's static
        buffers: consume them (``EpisodeReplay.add``) before the next collect."""
        with eval_mode(agent):
            if not graph:
                return self._run(agent, float(epsilon), False)
            g = self._graphs.lookup((agent,), ())
            if g is not None:
                self._eps_dev.fill_(float(epsilon))
                self._replay((g,), self.L)
                return self.batch()
            out = self._run(agent, float(epsilon), False)   # this call's episodes, and the warm-up
            off0 = self.offset
            g, _ = capture(self.env.device, lambda: self._run(agent, 0.0, True))
            self.offset = off0   # capture ran nothing
            self._graphs.store((agent,), (), None, g, self.L)
            return out

    def _run(self, agent, epsilon: float, dev_args: bool):
        env, L = self.env, self.L
        E, A = env.E, env.A
        env.reset()
        if env.tracker != "fresh":
            env.clear_tracker()
        self.active.fill_(1)
        R = self.ego_radius
        which = ("actor_map", "actor_vec", "critic_map", "critic_vec") if R is None else \
            ("actor_vec", "critic_map", "critic_vec")
        cv = self.canvas
        if cv is None:
            env.build_obs(out=self._slot(0), which=which)
        else:
            env.build_obs_canvas(cv, out=self._slot(0))
        if R is not None:
            env.build_obs_ego(R, out=self.so[0], dtype=self.ego_dtype)
        masks = self.avail
        if masks is not None:
            env.avail_actions(self.active, out=masks[0])
        h0 = agent.init_hidden()
        h0 = h0.reshape(1, -1).to(device=env.device, dtype=torch.float32)
        if self.hidden is None:
            self.hidden = torch.zeros((E * A, h0.shape[1]), dtype=torch.float32, device=env.device)
        h = h0.expand(E * A, -1)
        for t in range(L):
            so = self.so[t]
            q, h = agent(so.reshape(E * A, *so.shape[2:]), self.vo[t].reshape(E * A, -1), h)
            av = None if masks is None else masks[t]
            if dev_args:
                select_actions_eps_dev(q, self._eps_dev, self.seed, self._off_dev, t, avail=av, out=self.u[t].view(-1))
            else:
                select_actions_eps(q, epsilon, self.seed, self.offset, avail=av, out=self.u[t].view(-1))
            self.offset += 1
            if cv is None:
                env.step_episode(self.u[t], self.active, out=(self.r64[t], self.r_shaped[t], self.terminated[t]),
                                 filled=self.filled[t], obs_out=self._slot(t + 1), which=which)
            else:   # any map shapes: the step alone, then the stepped envs' canvas and vectors
                env.step_episode(self.u[t], self.active, out=(self.r64[t], self.r_shaped[t], self.terminated[t]),
                                 filled=self.filled[t], which=())
                env.build_obs_canvas(cv, rows=self.filled[t], out=self._slot(t + 1))
            if R is not None:   # the envs this step moved, those that just finished included
                env.build_obs_ego_masked(R, self.filled[t], out=self.so[t + 1], dtype=self.ego_dtype)
            if masks is not None:
                env.avail_actions(self.active, out=masks[t + 1])
        if dev_args:
            check(lib().mdl_counter_add(ptr(self._off_dev), L, stream_handle(env.device)), "mdl_counter_add")
        self.hidden.copy_(h)
        self.r.copy_(self.r64)   # fp64 -> float32, rounded once
        check(lib().mdl_read_state(env._h, None, None, None, ptr(self.episode_return), None, None,
                                   stream_handle(env.device)), "mdl_read_state")
        torch.sum(self.filled, dim=0, dtype=torch.int64, out=self.episode_length)
        return self.batch()
