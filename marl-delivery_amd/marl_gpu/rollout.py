"""Device-resident MAPPO rollout glue.

Replaces the host side of ``MAPPOTrainer.collect_rollouts`` (MAPPO/trainer.py:154-290):
the per-agent ``.item()`` + LabelEncoder decode, the Python env loop, shaping, tracker,
per-agent featurization with H2D copies, and the GAE loop.  Here the policy's logits
are sampled on the device (``sample_actions``), the engine steps and featurizes straight
into the rollout buffers, and GAE runs as one kernel (``gae``).  Only the actor/critic
forward passes are the caller's (torch modules, as in the reference).
"""
from __future__ import annotations

import numpy as np
import torch

from ._capture import Graphed, capture
from ._lib import check, lib, ptr, stream_handle
from .actions import ACTION_DIM, sample_actions, sample_actions_dev  # noqa: F401


def gae(rewards, values, next_value, dones, gamma=0.99, gae_lambda=0.95, out=None):
    """Advantages and returns exactly as MAPPO/trainer.py:266-276 computes them.

    rewards, values: float32 [T, n]; dones: bool/uint8 [T, n]; next_value: float32 [n].
    ``GAMMA * GAE_LAMBDA`` is formed in double and rounded once, as the reference's
    Python expression does before it meets a float32 tensor.
    """
    T, n = rewards.shape
    dev = rewards.device
    r = rewards.float().contiguous()
    v = values.float().contiguous()
    nv = next_value.reshape(n).float().contiguous()
    d = dones.to(torch.uint8).contiguous()
    if out is None:
        adv = torch.empty((T, n), dtype=torch.float32, device=dev)
        ret = torch.empty((T, n), dtype=torch.float32, device=dev)
    else:
        adv, ret = out
    g = float(np.float32(gamma))
    gl = float(np.float32(gamma * gae_lambda))
    check(lib().mdl_gae(ptr(r), ptr(v), ptr(nv), ptr(d), T, n, g, gl, ptr(adv), ptr(ret), stream_handle(dev)),
          "mdl_gae")
    return adv, ret


class MappoRollout(Graphed):
    """``collect_rollouts`` (MAPPO/trainer.py:154-290) on the device.

    env: a ``BatchedEnv`` built like the trainer's (tracker="mappo", shaping="mappo",
    max_other_robots=A-1, max_packages_obs=5, auto-reset on done).  actor(obs [E*A,6,H,W],
    vec [E*A,Dv]) -> logits [E*A, 15]; critic(gmap [E,4,H,W], gvec [E,Dg]) -> values [E]
    or [E, 1].  ``collect`` returns the reference's flattened batch.

    avail=True: each step's sampler takes the valid-action mask of the current state
    (``BatchedEnv.avail_actions``; ``sample_actions(avail=)``: the draw and the log-prob are those of
    the softmax over the available actions), and the masks are kept in ``mb_avail`` uint8
    [T, E, A, 15] so a learner applies the same mask when it recomputes log-probs.  The returned batch
    is unchanged in form.  avail=False (the default): nothing changes.

    obs_dtype: the element type of the observation buffers (``mb_obs``, ``mb_vector_obs``,
    ``mb_global_states``, ``mb_global_vector`` and ``next_obs``): torch.float32 (the default), or
    torch.float16 / torch.bfloat16 -- the engine then writes the float32 observations rounded once to
    nearest-even (``BatchedEnv.build_obs(dtype=)``), half the bytes, and actor and critic receive
    tensors of that type (a policy under autocast, or one that casts its inputs).  Rewards, values,
    log-probs, advantages and returns stay float32.

    ego_radius: None (the default: nothing changes), or a radius R in 1..15 -- the actor then sees each
    robot's ``K x K`` window of its map, centred on the robot (K = 2R + 1, ``BatchedEnv.build_obs_ego``):
    ``mb_obs`` and ``next_obs["actor_map"]`` are [.., A, 6, K, K] in ``obs_dtype``, the actor receives
    obs [E*A, 6, K, K], and every step is ``step_obs`` of the other three tensors followed by
    ``build_obs_ego`` into the next slot (the first observation likewise).  The critic keeps the full
    map, so the envs must still share one map shape -- unless ``canvas`` is given.

    canvas: None (the default: nothing changes), or (Hc, Wc) with ``ego_radius`` (ValueError without it)
    -- the critic then sees its map on that fixed canvas (``BatchedEnv.build_obs_canvas``: the map in the
    top-left corner, off-map cells obstacles), so the engine may mix map shapes: one policy collects on
    several maps at once.  ``mb_global_states`` and ``next_obs["critic_map"]`` are [.., 4, Hc, Wc], the
    critic receives gmap [E, 4, Hc, Wc], and every step is ``step(auto_reset=True)``,
    ``build_obs_canvas`` into the next slot, then ``build_obs_ego``.  The canvas must cover every map.
    """

    def __init__(self, env, rollout_steps: int, seed: int = 0, gamma: float = 0.99, gae_lambda: float = 0.95,
                 avail: bool = False, obs_dtype: torch.dtype = torch.float32, ego_radius: int | None = None,
                 canvas=None):
        self.env = env
        self.ego_radius = None if ego_radius is None else env._ego_radius(ego_radius)
        if canvas is not None and self.ego_radius is None:
            raise ValueError("MappoRollout: canvas needs ego_radius (the actor's full map has no shape "
                             "common to several maps)")
        self.canvas = None if canvas is None else env._canvas(canvas)
        if obs_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"obs_dtype must be torch.float32, torch.float16 or torch.bfloat16, not {obs_dtype}")
        self.obs_dtype = obs_dtype
        self.T = int(rollout_steps)
        self.seed = int(seed)
        self._init_graphs(env.device)
        self.gamma, self.gae_lambda = gamma, gae_lambda
        E, A = env.E, env.A
        H, W = env.single_map_shape("MappoRollout") if self.canvas is None else self.canvas
        dev = env.device
        f = dict(dtype=torch.float32, device=dev)
        T = self.T
        o = dict(dtype=obs_dtype, device=dev)
        if self.ego_radius is None:
            self.mb_obs = torch.zeros((T, E, A, 6, H, W), **o)
        else:
            K = 2 * self.ego_radius + 1
            self.mb_obs = torch.zeros((T, E, A, 6, K, K), **o)
        self.mb_vector_obs = torch.zeros((T, E, A, env.actor_vec_dim), **o)
        self.mb_global_states = torch.zeros((T, E, 4, H, W), **o)
        self.mb_global_vector = torch.zeros((T, E, env.critic_vec_dim), **o)
        self.mb_actions = torch.zeros((T, E, A), dtype=torch.uint8, device=dev)
        self.mb_log_probs = torch.zeros((T, E, A), **f)
        self.mb_rewards = torch.zeros((T, E), **f)
        self.mb_dones = torch.zeros((T, E), dtype=torch.uint8, device=dev)
        self.mb_values = torch.zeros((T, E), **f)
        if self.canvas is None:
            self.next_obs = env.obs_buffers(E, H, W, obs_dtype)
        else:
            self.next_obs = env.canvas_buffers(self.canvas, E, obs_dtype)
        if self.ego_radius is not None:
            self.next_obs["actor_map"] = env.ego_buffers(self.ego_radius, E, obs_dtype)
        self._r_env = torch.zeros(E, dtype=torch.float64, device=dev)
        self._graph_out = None
        self.mb_avail = torch.ones((T, E, A, ACTION_DIM), dtype=torch.uint8, device=dev) if avail else None

    def _slot(self, k):
        return dict(actor_map=self.mb_obs[k], actor_vec=self.mb_vector_obs[k], critic_map=self.mb_global_states[k],
                    critic_vec=self.mb_global_vector[k])

    @torch.no_grad()
    def collect(self, actor, critic, graph: bool = False):
        """One rollout of ``rollout_steps`` env steps.  graph=True: the first call runs
        eagerly and captures the whole rollout (policy forwards, sampling, steps,
        observations, GAE) as one hipGraph; later calls with the same actor/critic replay
        it -- bit-identical to eager calls, in any interleaving (the graph rule, ``_capture``).
        The returned tensors are the graph's static buffers: consume them before the next
        collect."""
        if not graph:
            return self._run(actor, critic, False)
        g = self._graphs.lookup((actor, critic), ())
        if g is not None:
            self._replay((g,), self.T)
            return self._graph_out
        out = self._run(actor, critic, False)        # this call's rollout, and the warm-up
        off0 = self.offset
        g, self._graph_out = capture(self.env.device, lambda: self._run(actor, critic, True))
        self.offset = off0   # capture ran nothing
        self._graphs.store((actor, critic), (), None, g, self.T)
        return out

    def _run(self, actor, critic, dev_offset: bool):
        env, T = self.env, self.T
        E, A = env.E, env.A
        R = self.ego_radius
        # with a radius the actor map is the window builder's
        which = ("actor_vec", "critic_map", "critic_vec") if R is not None else \
            ("actor_map", "actor_vec", "critic_map", "critic_vec")
        cv = self.canvas
        if cv is None:
            env.build_obs(out=self._slot(0), which=which, dtype=self.obs_dtype)   # current obs = f(current state, tracker)
        else:
            env.build_obs_canvas(cv, out=self._slot(0), dtype=self.obs_dtype)
        if R is not None:
            env.build_obs_ego(R, out=self.mb_obs[0], dtype=self.obs_dtype)
        for step in range(T):
            obs = self.mb_obs[step]
            logits = actor(obs.reshape(E * A, *obs.shape[2:]), self.mb_vector_obs[step].reshape(E * A, -1))
            acts_lp = (self.mb_actions[step].view(-1), self.mb_log_probs[step].view(-1))
            av = None if self.mb_avail is None else env.avail_actions(out=self.mb_avail[step])
            if dev_offset:
                sample_actions_dev(logits, self.seed, self._off_dev, step, out=acts_lp, avail=av)
            else:
                sample_actions(logits, self.seed, self.offset, out=acts_lp, avail=av)
            self.offset += 1
            self.mb_values[step] = critic(self.mb_global_states[step], self.mb_global_vector[step]).reshape(E)
            # step + the next observations in one launch (MAPPO/trainer.py:229-286)
            nxt = self._slot(step + 1) if step + 1 < T else self.next_obs
            if cv is None:
                env.step_obs(self.mb_actions[step], auto_reset=True,
                             out=(self._r_env, self.mb_rewards[step], self.mb_dones[step]),
                             obs_out=nxt, which=which, obs_dtype=self.obs_dtype)
            else:   # any map shapes: the step, then the canvas and the vectors of the new state
                env.step(self.mb_actions[step], auto_reset=True,
                         out=(self._r_env, self.mb_rewards[step], self.mb_dones[step]))
                env.build_obs_canvas(cv, out=nxt, dtype=self.obs_dtype)
            if R is not None:
                env.build_obs_ego(R, out=nxt["actor_map"], dtype=self.obs_dtype)
        if dev_offset:
            check(lib().mdl_counter_add(ptr(self._off_dev), T, stream_handle(env.device)), "mdl_counter_add")
        next_value = critic(self.next_obs["critic_map"], self.next_obs["critic_vec"]).reshape(E)
        adv, ret = gae(self.mb_rewards, self.mb_values, next_value, self.mb_dones, self.gamma, self.gae_lambda)
        H, W = self.mb_global_states.shape[-2:]
        return (self.mb_obs.reshape(-1, *self.mb_obs.shape[3:]), self.mb_vector_obs.reshape(T * E * A, -1),
                self.mb_global_states.reshape(T * E, 4, H, W), self.mb_global_vector.reshape(T * E, -1),
                self.mb_actions.reshape(-1).long(), self.mb_log_probs.reshape(-1),
                adv.reshape(T * E, 1).repeat(1, A).reshape(-1), ret.reshape(-1), self.mb_rewards)
