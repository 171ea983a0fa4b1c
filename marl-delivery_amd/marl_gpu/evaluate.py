"""Device-resident evaluation (the counterpart of ``evaluation.run_eval``, evaluation.py:9-66).

The reference evaluates an agent episode by episode: build an ``Environment`` seeded
``seed + ep``, ``init_agents``, then ``get_actions`` / ``env.step`` until done, and read the
episode's ``total_reward`` and its delivered packages.  Here the episodes are the envs of one
``BatchedEnv``: every env runs one episode from a fresh reset, the envs whose episode still runs
are a mask on the device (``step_episode`` clears a finished env's byte), the greedy agent takes
that mask (``greedy_actions_masked``), and the results come from one small launch
(``episode_results``).  Nothing inside the loop synchronises with the host, so the loop can be
captured as a hipGraph.  ``summary()`` is the one host read.
"""
from __future__ import annotations

import numpy as np
import torch

from ._capture import Graphed, capture, eval_mode
from ._lib import check, lib, ptr, stream_handle
from .actions import ACTION_DIM, sample_actions, sample_actions_dev, select_actions_eps

# randomagent.py:16-17 in the engine's action codes (move code | op << 3)
_RANDOM_MOVES = np.array([3, 4, 1, 2, 0], np.uint8)   # 'U', 'D', 'L', 'R', 'S'


def summarize(rewards, delivered, n_packages) -> dict:
    """``run_eval``'s result dict from the per-episode lists, computed exactly as
    evaluation.py:52-66 computes it (Python lists, numpy on the host), so equal per-episode
    values give bit-equal means and deviations."""
    rewards = [float(x) for x in rewards]
    delivered = [int(x) for x in delivered]
    delivery_rate = []
    for n_delivered in delivered:
        rate = 0
        if n_packages > 0:
            rate = (n_delivered / n_packages) * 100
        delivery_rate.append(rate)
    return {
        "rewards": rewards,
        "delivered": delivered,
        "delivery_rate": delivery_rate,
        "mean_reward": np.mean(rewards) if rewards else 0,
        "std_reward": np.std(rewards) if rewards else 0,
        "mean_delivered": np.mean(delivered) if delivered else 0,
        "std_delivered": np.std(delivered) if delivered else 0,
        "mean_delivery_rate": np.mean(delivery_rate) if delivery_rate else 0,
        "std_delivery_rate": np.std(delivery_rate) if delivery_rate else 0,
    }


def random_action_tape(seed: int, n_episodes: int, n_robots: int, max_time_steps: int) -> np.ndarray:
    """The random agent's actions (randomagent.py:16-22) for ``n_episodes`` full-length episodes run
    one after the other under ``np.random.seed(seed)`` (evaluation.py:80, :12-47): uint8
    [max_time_steps, n_episodes, n_robots] in the "codes" action format.  Per episode, per step, per
    robot the agent draws ``choice(['U','D','L','R','S'])`` then ``choice(['0','1','2'])``; a
    ``choice`` over n items without weights is one ``randint(0, n)`` of the same stream, which is
    what is drawn here, on a private ``RandomState(seed)``.  The tape lines up with the reference
    only while every episode runs all ``max_time_steps`` steps (``run_eval`` checks that)."""
    rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    n = int(n_episodes) * int(max_time_steps) * int(n_robots)
    mv = np.empty(n, np.int64)
    op = np.empty(n, np.int64)
    randint = rs.randint
    for i in range(n):
        mv[i] = randint(0, 5)
        op[i] = randint(0, 3)
    codes = (_RANDOM_MOVES[mv] | (op.astype(np.uint8) << 3)).reshape(n_episodes, max_time_steps, n_robots)
    return np.ascontiguousarray(codes.transpose(1, 0, 2))


class Evaluator(Graphed):
    """One evaluation episode per env of ``env`` (a ``BatchedEnv`` whose envs share one map shape;
    build it with tracker="fresh" as the evaluation's agents use -- a stale tracker is cleared before
    the reset).  ``seed`` keys the sampler of a stochastic policy.  Every run resets the envs, which
    draws each env's next layout from its own stream: the first run on a newly built engine plays
    the reference's episode of each seed (``Environment(seed)`` then ``env.reset()``,
    evaluation.py:13-20), a second run the episodes after them.

    ``run(agent)`` takes
      "greedy"                    greedyagent.py on the device (``greedy_actions_masked``);
      a uint8 tensor [L', E, A]   an action tape in the "codes" format, L' >= the run's steps: step k
                                  feeds ``tape[k]`` (state-independent agents, ``random_action_tape``);
      a callable                  ``policy(actor_map [E*A, 6, H, W], actor_vec [E*A, Dv]) -> logits
                                  [E*A, n_actions]`` (``ActorNetwork.forward``, MAPPO/networks.py:52, as
                                  agent.py:86-104 calls it), actions as trainer ints.
    The policy's forward also runs on the finished envs' stale rows (as ``QmixCollector``'s agent
    does); their actions are never used, the engine does not step them.

    ego_radius=R (1..15, K = 2R + 1; policies only, the greedy and tape kinds ignore it): the policy
    is called as ``policy(actor_ego [E*A, 6, K, K], actor_vec [E*A, Dv])`` with each robot's window of
    its actor map (``BatchedEnv.build_obs_ego``) in ``ego_dtype`` (torch.float32, float16 or bfloat16;
    actor_vec stays float32).  Each step is then ``step_episode`` for the vectors and
    ``build_obs_ego_masked`` over the envs it stepped."""

    def __init__(self, env, seed: int = 0, ego_radius: int | None = None, ego_dtype: torch.dtype = torch.float32):
        self._hw = env.single_map_shape("Evaluator")
        self.ego_radius = None if ego_radius is None else env._ego_radius(ego_radius)
        self.ego_dtype = ego_dtype
        if self.ego_radius is not None:
            env.ego_buffers(self.ego_radius, 0, ego_dtype)   # raises on a dtype the builder does not write
        self.env = env
        self.seed = int(seed)
        self._init_graphs(env.device)
        E, A, dev = env.E, env.A, env.device
        self.active = torch.zeros(E, dtype=torch.uint8, device=dev)
        self.filled = torch.zeros(E, dtype=torch.uint8, device=dev)   # the envs the last step moved (windows)
        self.actions = torch.zeros((E, A), dtype=torch.uint8, device=dev)
        self.rewards = torch.zeros(E, dtype=torch.float64, device=dev)
        self.delivered = torch.zeros(E, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(E, dtype=torch.int32, device=dev)
        self._log_probs = torch.zeros(E * A, dtype=torch.float32, device=dev)   # the sampler's second output
        self._obs = None              # the policy's observation buffers, used in place
        self.avail = None             # uint8 [E, A, 15], the last step's mask of a run with avail=True
        self._masked = False

    # ------------------------------------------------------------------ results
    def results(self) -> dict:
        """Device tensors of the last run: rewards f64 [E] (each env's ``total_reward``), delivered
        int32 [E], steps int32 [E] (its ``t``) and finished uint8 [E] (its episode ended)."""
        return dict(rewards=self.rewards, delivered=self.delivered, steps=self.steps,
                    finished=(self.active == 0).to(torch.uint8))

    def summary(self) -> dict:
        """``run_eval``'s dict (evaluation.py:56-66) of the last run: one device-to-host copy, one
        synchronisation, then ``summarize`` on the host."""
        host = torch.stack((self.rewards, self.delivered.double())).cpu()
        return summarize(host[0].tolist(), [int(x) for x in host[1].tolist()], self.env.P)

    # ------------------------------------------------------------------ the run
    def _kind(self, agent):
        if isinstance(agent, str):
            if agent != "greedy":
                raise ValueError(f"Evaluator: unknown agent {agent!r} (\"greedy\", an action tape or a policy)")
            return "greedy"
        if isinstance(agent, torch.Tensor):
            return "tape"
        if callable(agent):
            return "policy"
        raise TypeError("Evaluator: agent must be \"greedy\", a uint8 action tape [L, E, A] or a callable policy")

    @torch.no_grad()
    def run(self, agent, max_steps: int | None = None, deterministic: bool = True, graph: bool = False,
            graph_steps: int = 50, avail: bool = False) -> dict:
        """One episode of at most L = min(max_steps or env.T, env.T) steps in every env, from a fresh
        reset; returns ``results()``.  deterministic (policies only): the lowest index among the
        largest logits (``select_actions_eps`` at epsilon 0); otherwise ``sample_actions`` at
        (seed, offset), the offset advancing by one per step.  A policy module runs in eval mode
        and its mode is restored.  avail (policies only): the selection, or the sampler, takes the
        valid-action mask of each state (``BatchedEnv.avail_actions`` with the running-env mask, one
        small launch per step), so the policy never plays an action that is certain to equal a
        simpler one.

        graph=True: the first call runs eagerly, then captures min(L, graph_steps) steps as one
        hipGraph (and the L mod chunk remaining steps as a second one); later calls with the same
        agent object, its parameters at the same addresses, and the same arguments replay them --
        bit-identical to the eager run, in any interleaving (the graph rule, ``_capture``).  A tape's
        graph holds all L steps."""
        env = self.env
        kind = self._kind(agent)
        L = min(int(max_steps) if max_steps else env.T, env.T)
        if L < 1:
            raise ValueError("Evaluator: max_steps must be >= 1")
        if kind == "tape":
            E, A = env.E, env.A
            if agent.dim() != 3 or agent.shape[1] != E or agent.shape[2] != A:
                raise ValueError(f"Evaluator: an action tape must be [L, {E}, {A}]")
            if agent.shape[0] < L:
                raise ValueError(f"Evaluator: the action tape holds {agent.shape[0]} steps, the run needs {L}")
            if agent.dtype != torch.uint8 or not agent.is_cuda or agent.get_device() != env.device.index \
                    or not agent.is_contiguous():
                raise TypeError(f"Evaluator: an action tape must be a contiguous uint8 tensor on {env.device}")
        det = bool(deterministic)
        self._masked = bool(avail) and kind == "policy"
        with eval_mode(agent):
            if not graph:
                self._begin(kind)
                self._steps(kind, agent, 0, L, det, False)
                self._end()
                return self.results()
            chunk = L if kind == "tape" else min(L, int(graph_steps))
            if chunk < 1:
                raise ValueError("Evaluator: graph_steps must be >= 1")
            # a graph reads the agent's parameters (or the tape) in place: replay only for the very same object
            owners, values = (agent,), (kind, L, chunk, det, self._masked)
            g = self._graphs.lookup(owners, values, "chunk")
            self._begin(kind)
            if g is not None:
                g_rem = self._graphs.lookup(owners, values, "rest")
                graphs = (g,) * (L // chunk) + ((g_rem,) if g_rem is not None else ())
                self._replay(graphs, L if kind == "policy" and not det else 0)   # only the sampler draws
                self._end()
                return self.results()
            self._steps(kind, agent, 0, L, det, False)   # this call's episodes, and the warm-up
            self._end()
            for slot, n in (("chunk", chunk), ("rest", L % chunk)):
                if n:   # n steps as one hipGraph; a tape's graph starts at step 0 (it holds the whole run)
                    g, _ = capture(env.device, lambda: self._steps(kind, agent, 0, n, det, True))
                    self._graphs.store(owners, values, slot, g, n)
            return self.results()

    def _begin(self, kind):
        env = self.env
        if env.tracker != "fresh":
            env.clear_tracker()
        env.reset()
        self.active.fill_(1)
        if kind == "greedy":
            env.greedy_init()
        elif kind == "policy":
            R = self.ego_radius
            if self._obs is None:
                H, W = self._hw
                f = dict(dtype=torch.float32, device=env.device)
                amap = torch.empty((env.E, env.A, 6, H, W), **f) if R is None else \
                    env.ego_buffers(R, dtype=self.ego_dtype)
                self._obs = dict(actor_map=amap, actor_vec=torch.empty((env.E, env.A, env.actor_vec_dim), **f))
            if R is None:
                env.build_obs(out=self._obs, which=("actor_map", "actor_vec"))
            else:
                env.build_obs(out=self._obs, which=("actor_vec",))
                env.build_obs_ego(R, out=self._obs["actor_map"], dtype=self.ego_dtype)
            if self._masked and self.avail is None:
                self.avail = torch.ones((env.E, env.A, ACTION_DIM), dtype=torch.uint8, device=env.device)

    def _steps(self, kind, agent, k0, n, deterministic, dev_offset):
        """Steps k0 .. k0+n-1 of the run.  dev_offset (under capture): the sampler's offset is the
        device counter plus the step's index in this chunk, and the counter advances by n at the end."""
        env = self.env
        E, A = env.E, env.A
        for k in range(n):
            if kind == "greedy":
                env.greedy_actions_masked(self.active, out=self.actions)
                env.step_episode(self.actions, self.active, action_format="codes", which=())
            elif kind == "tape":
                env.step_episode(agent[k0 + k], self.active, action_format="codes", which=())
            else:
                om, ov = self._obs["actor_map"], self._obs["actor_vec"]
                logits = agent(om.reshape(E * A, *om.shape[2:]), ov.reshape(E * A, -1))
                acts = self.actions.view(-1)
                av = env.avail_actions(self.active, out=self.avail) if self._masked else None
                if deterministic:
                    select_actions_eps(logits, 0.0, self.seed, 0, avail=av, out=acts)
                elif dev_offset:
                    sample_actions_dev(logits, self.seed, self._off_dev, k, out=(acts, self._log_probs), avail=av)
                else:
                    sample_actions(logits, self.seed, self.offset, out=(acts, self._log_probs), avail=av)
                    self.offset += 1
                if self.ego_radius is None:
                    env.step_episode(self.actions, self.active, action_format="int", obs_out=self._obs,
                                     which=("actor_map", "actor_vec"))
                else:
                    env.step_episode(self.actions, self.active, action_format="int", filled=self.filled,
                                     obs_out=self._obs, which=("actor_vec",))
                    env.build_obs_ego_masked(self.ego_radius, self.filled, out=om, dtype=self.ego_dtype)
        if dev_offset and kind == "policy" and not deterministic:
            check(lib().mdl_counter_add(ptr(self._off_dev), n, stream_handle(env.device)), "mdl_counter_add")

    def _end(self):
        self.env.episode_results(out=(self.rewards, self.delivered, self.steps))


def run_eval(agent_type: str, env_config: dict, num_episodes: int, policy=None, deterministic: bool | None = None,
             agent_seed: int | None = None, graph: bool = False, ego_radius: int | None = None,
             ego_dtype: torch.dtype = torch.float32) -> dict:
    """``evaluation.run_eval`` (evaluation.py:9-66) with the ``num_episodes`` episodes as the envs of
    one ``BatchedEnv``: env ``ep`` is seeded ``env_config['seed'] + ep``, tracker "fresh".
    env_config: map, max_time_steps, n_agents, n_packages, seed (evaluation.py:94-100).
    agent_type "greedy"; "random" (the tape of ``random_action_tape(agent_seed, ...)``, agent_seed
    defaulting to env_config['seed'] as evaluation.py:80 seeds numpy; raises RuntimeError if an
    episode ended before max_time_steps, because the reference's stream would then be shorter for
    that episode and the tape would no longer line up); "mappo" (``policy``, sampled unless
    ``deterministic`` is given: evaluation.py:40-42).  ego_radius / ego_dtype: the policy takes actor-map
    windows (``Evaluator``).  Returns the reference's result dict."""
    from .engine import BatchedEnv
    if agent_type not in ("greedy", "random", "mappo"):
        raise ValueError(f"Unknown agent type: {agent_type}")
    if agent_type == "mappo" and policy is None:
        raise ValueError("run_eval: agent_type \"mappo\" needs a policy")
    E, T = int(num_episodes), int(env_config["max_time_steps"])
    if E < 1:
        return summarize([], [], int(env_config["n_packages"]))
    base = int(env_config["seed"])
    seed = base if agent_seed is None else int(agent_seed)
    env = BatchedEnv(env_config["map"], E, int(env_config["n_agents"]), int(env_config["n_packages"]), T,
                     seeds=[base + ep for ep in range(E)], tracker="fresh")
    try:
        ev = Evaluator(env, seed=seed, ego_radius=ego_radius, ego_dtype=ego_dtype)
        if agent_type == "greedy":
            ev.run("greedy", graph=graph)
        elif agent_type == "random":
            tape = torch.from_numpy(random_action_tape(seed, E, env.A, T)).to(env.device)
            res = ev.run(tape, graph=graph)
            if int((res["steps"] != T).sum()):
                raise RuntimeError("run_eval: a random episode ended before max_time_steps; the reference draws "
                                   "fewer actions for it, so the action tape does not reproduce its stream")
        else:
            ev.run(policy, deterministic=False if deterministic is None else bool(deterministic), graph=graph)
        return ev.summary()
    finally:
        env.close()
