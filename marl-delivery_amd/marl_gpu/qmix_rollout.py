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

from ._lib import check, lib, ptr, stream_handle

ACTION_DIM = 15  # QMIX/trainer.py: num_move_actions * num_pkg_ops


def _q_avail(q, avail):
    if q.dtype != torch.float32 or not q.is_contiguous():
        q = q.float().contiguous()
    if q.dim() != 2:
        raise ValueError("q must be [rows, n_actions]")
    if avail is not None:
        if avail.shape != q.shape:
            raise ValueError("avail must have q's shape")
        if avail.dtype != torch.uint8 or not avail.is_contiguous():
            avail = avail.to(torch.uint8).contiguous()
    return q, avail


def select_actions_eps(q: torch.Tensor, epsilon: float, seed: int, offset: int, avail=None, out=None):
    """Epsilon-greedy selection over Q-values (QMIX/trainer.py:298-319).

    q: float32 [N, n_actions] on the device; avail: bool/uint8 of the same shape or None
    (= every action available).  Returns actions uint8 [N].  A row explores with
    probability epsilon and then takes a uniformly drawn available action; otherwise it
    takes the first available action with the largest q.  The draw is the library's own
    Philox4x32-10 stream keyed by (seed, offset, row) -- include/mdl_engine.h states it
    exactly --: deterministic, independent of launch shape."""
    q, avail = _q_avail(q, avail)
    N, n_act = q.shape
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=q.device)
    check(lib().mdl_select_actions_eps(ptr(q), ptr(avail), N, n_act, float(epsilon), seed & (2**64 - 1),
                                       offset & (2**64 - 1), ptr(out), stream_handle(q.device)),
          "mdl_select_actions_eps")
    return out


def select_actions_eps_dev(q: torch.Tensor, epsilon_dev: torch.Tensor, seed: int, offset_dev: torch.Tensor,
                           offset_add: int, avail=None, out=None):
    """``select_actions_eps`` with epsilon (float32 tensor [1]) and the offset base (uint64
    bits in an int64 tensor [1]; the offset is ``offset_dev[0] + offset_add``) read on the
    device, so the launch can live in a replayed hipGraph."""
    q, avail = _q_avail(q, avail)
    N, n_act = q.shape
    if epsilon_dev.dtype != torch.float32 or offset_dev.dtype != torch.int64:
        raise TypeError("epsilon_dev must be float32 and offset_dev int64 (uint64 bits)")
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=q.device)
    check(lib().mdl_select_actions_eps_dev(ptr(q), ptr(avail), N, n_act, ptr(epsilon_dev), seed & (2**64 - 1),
                                           ptr(offset_dev), offset_add & (2**64 - 1), ptr(out),
                                           stream_handle(q.device)), "mdl_select_actions_eps_dev")
    return out


class QmixCollector:
    """``collect_data_iteration`` (QMIX/trainer.py:333-528) on the device: one episode per env.

    env: a ``BatchedEnv`` built like the trainer's (shaping="qmix"; tracker="fresh", or a
    stale tracker, which ``collect`` clears after the reset as QMIX/trainer.py:523-526 does).
    agent(so [E*A, 6, H, W], vo [E*A, Dv], h [E*A, Hd]) -> (q [E*A, n_actions], h' [E*A, Hd]),
    with ``agent.init_hidden()`` -> [1, Hd] as the reference's ``AgentNetwork``.

    Time-major buffers, L = min(episode_limit, env.T):
      so [L+1, E, A, 6, H, W], vo [L+1, E, A, Dv], gs [L+1, E, 4, H, W], gv [L+1, E, Dg]
      (slot t = the observations before step t, slot t+1 = after it), u uint8 [L, E, A],
      r float32 [L, E] (the fp64 global reward rounded once, as the reference's float32
      buffer does; r64 keeps the fp64 values), r_shaped float32 [L, E], terminated and
      filled uint8 [L, E], hidden [E*A, Hd] (the last hidden states).
    Rows of an env past its episode's end (filled == 0) are not written: they hold whatever
    an earlier collect left there.

    One deviation from the reference: the agent also runs on the finished envs (the
    reference shrinks its batch instead).  Their actions and hidden states are ignored --
    the engine does not step them -- so the finished envs cost forward-pass time only.
    """

    def __init__(self, env, episode_limit: int, seed: int = 0):
        self.env = env
        self.L = L = min(int(episode_limit), env.T)
        if L < 1:
            raise ValueError("QmixCollector: episode_limit must be >= 1")
        self.seed = int(seed)
        self.offset = 0
        E, A = env.E, env.A
        if env._shape_run_end[0] < E:
            raise ValueError("QmixCollector: the engine's envs mix map shapes (build one engine per map shape)")
        H, W = env.grids[int(env.env_map[0])].shape
        dev = env.device
        f = dict(dtype=torch.float32, device=dev)
        b = dict(dtype=torch.uint8, device=dev)
        self.so = torch.zeros((L + 1, E, A, 6, H, W), **f)
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
        self._graph = None            # hipGraph of one whole collect (collect(graph=True))
        self._graph_key = None        # (agent, parameter addresses) the graph was captured with
        self._off_dev = torch.zeros(1, dtype=torch.int64, device=dev)   # selection offset base (uint64 bits)
        self._eps_dev = torch.zeros(1, **f)

    def _slot(self, k):
        return dict(actor_map=self.so[k], actor_vec=self.vo[k], critic_map=self.gs[k], critic_vec=self.gv[k])

    def batch(self):
        """The buffers of the last collect (the collector's own tensors, not copies)."""
        return dict(so=self.so, vo=self.vo, gs=self.gs, gv=self.gv, u=self.u, r=self.r, r64=self.r64,
                    r_shaped=self.r_shaped, terminated=self.terminated, filled=self.filled, hidden=self.hidden,
                    episode_return=self.episode_return, episode_length=self.episode_length)

    @torch.no_grad()
    def collect(self, agent, epsilon: float, graph: bool = False):
        """One episode of at most L steps in every env, from a fresh reset.  Returns ``batch()``:
        the buffers plus episode_return (fp64 [E], each env's ``total_reward``) and
        episode_length (int64 [E], ``filled.sum(0)``).  The forward passes run with the agent
        in eval mode (if it has ``eval`` / ``train``) and its mode is restored afterwards, as
        QMIX/trainer.py:287-289 does.  Nothing inside the loop synchronises with the host.

        graph=True: the first call runs eagerly and captures the whole collect (reset,
        forwards, selection, steps, observations) as one hipGraph; later calls with the same
        agent replay it -- bit-identical to eager calls (epsilon and the selection's offset
        base live on the device).  The returned tensors are the graph's static buffers:
        consume them (``EpisodeReplay.add``) before the next collect."""
        was_training = bool(getattr(agent, "training", False))
        if hasattr(agent, "eval"):
            agent.eval()
        try:
            if not graph:
                return self._run(agent, float(epsilon), False)
            # the graph reads the module's parameters in place: replay only for the very same module
            # whose parameters still live at the captured addresses (MappoRollout.collect's rule)
            ptrs = tuple(q.data_ptr() for q in agent.parameters()) if hasattr(agent, "parameters") else ()
            k0 = self._graph_key
            if self._graph is not None and k0[0] is agent and k0[1] == ptrs:
                self._eps_dev.fill_(float(epsilon))
                self._graph.replay()
                self.offset += self.L
                return self.batch()
            out = self._run(agent, float(epsilon), False)   # this call's episodes, and the warm-up
            self._capture(agent, (agent, ptrs))
            return out
        finally:
            if was_training and hasattr(agent, "train"):
                agent.train()

    def _capture(self, agent, key):
        dev = self.env.device
        torch.cuda.synchronize(dev)
        self._off_dev.fill_(self.offset)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        off0 = self.offset
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._run(agent, 0.0, True)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        self.offset = off0   # capture ran nothing
        self._graph, self._graph_key = g, key

    def _run(self, agent, epsilon: float, dev_args: bool):
        env, L = self.env, self.L
        E, A = env.E, env.A
        env.reset()
        if env.tracker != "fresh":
            env.clear_tracker()
        self.active.fill_(1)
        env.build_obs(out=self._slot(0))
        h0 = agent.init_hidden()
        h0 = h0.reshape(1, -1).to(device=env.device, dtype=torch.float32)
        if self.hidden is None:
            self.hidden = torch.zeros((E * A, h0.shape[1]), dtype=torch.float32, device=env.device)
        h = h0.expand(E * A, -1)
        for t in range(L):
            so = self.so[t]
            q, h = agent(so.reshape(E * A, *so.shape[2:]), self.vo[t].reshape(E * A, -1), h)
            if dev_args:
                select_actions_eps_dev(q, self._eps_dev, self.seed, self._off_dev, t, out=self.u[t].view(-1))
            else:
                select_actions_eps(q, epsilon, self.seed, self.offset, out=self.u[t].view(-1))
            self.offset += 1
            env.step_episode(self.u[t], self.active, out=(self.r64[t], self.r_shaped[t], self.terminated[t]),
                             filled=self.filled[t], obs_out=self._slot(t + 1))
        if dev_args:
            check(lib().mdl_counter_add(ptr(self._off_dev), L, stream_handle(env.device)), "mdl_counter_add")
        self.hidden.copy_(h)
        self.r.copy_(self.r64)   # fp64 -> float32, rounded once
        check(lib().mdl_read_state(env._h, None, None, None, ptr(self.episode_return), None, None,
                                   stream_handle(env.device)), "mdl_read_state")
        torch.sum(self.filled, dim=0, dtype=torch.int64, out=self.episode_length)
        return self.batch()


class EpisodeReplay:
    """The reference's episode ``ReplayBuffer`` (QMIX/networks.py:209-318) as a time-major ring
    of ``capacity`` episodes in plain torch ops, on the device of the template's tensors.

    ``collector``: a ``QmixCollector`` or one of its batches (a dict with so, vo, gs, gv, u, r,
    terminated, filled) -- the template for shapes, dtypes and device.

    ``add`` stores a batch's E episodes in env order; the reference stores each episode when it
    terminates, i.e. in termination order.  Only the eviction order inside one batch differs.
    """

    FIELDS = ("so", "vo", "gs", "gv", "u", "r", "terminated", "filled")

    def __init__(self, capacity: int, collector, n_actions: int = ACTION_DIM):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("EpisodeReplay: capacity must be >= 1")
        self.n_actions = int(n_actions)
        tpl = collector if isinstance(collector, dict) else collector.batch()
        self.buf = {}
        for k in self.FIELDS:
            t = tpl[k]
            self.buf[k] = torch.zeros((t.shape[0], self.capacity) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
        self.L = tpl["u"].shape[0]
        self.device = tpl["u"].device
        self.size = 0
        self.idx = 0

    def __len__(self):
        return self.size

    def add(self, batch):
        """Store the E episodes of ``batch`` (env order) in the next E ring slots, evicting the
        oldest episodes once the ring is full."""
        E = batch["u"].shape[1]
        first = max(0, E - self.capacity)   # a batch larger than the ring keeps its last `capacity` episodes
        slots = (torch.arange(first, E) + self.idx) % self.capacity
        slots = slots.to(self.device)
        for k in self.FIELDS:
            self.buf[k][:, slots] = batch[k][:, first:]
        self.idx = (self.idx + E) % self.capacity
        self.size = min(self.capacity, self.size + E)

    def sample(self, batch_size: int, generator=None):
        """``batch_size`` distinct stored episodes as the reference's dictionary
        (QMIX/networks.py:299-314), episode-major: so / vo / gs / gv and their ``_next`` forms
        ([B, L, ...]; ``*_next`` is the same gathered tensor shifted by one slot, not a second
        copy), u int64 [B, L, A, 1], r [B, L, 1], avail_u / avail_u_next (all ones, [B, L, A,
        n_actions]), terminated and padded (= 1 - filled) float32 [B, L, 1]."""
        B = int(batch_size)
        if B < 1 or self.size < B:
            raise ValueError(f"EpisodeReplay holds {self.size} episodes, cannot sample {B}")
        gdev = generator.device if generator is not None else torch.device("cpu")
        idx = torch.randperm(self.size, generator=generator, device=gdev)[:B].to(self.device)
        L = self.L
        out = {}
        for k in ("so", "vo", "gs", "gv"):
            x = self.buf[k][:, idx].transpose(0, 1)   # [B, L+1, ...]
            out[k] = x[:, :L]
            out[k + "_next"] = x[:, 1:]
        A = self.buf["u"].shape[2]
        out["u"] = self.buf["u"][:, idx].transpose(0, 1).long().unsqueeze(-1)
        out["r"] = self.buf["r"][:, idx].transpose(0, 1).unsqueeze(-1)
        ones = torch.ones((), dtype=torch.float32, device=self.device).expand(B, L, A, self.n_actions)
        out["avail_u"] = ones
        out["avail_u_next"] = ones
        out["terminated"] = self.buf["terminated"][:, idx].transpose(0, 1).float().unsqueeze(-1)
        out["padded"] = 1.0 - self.buf["filled"][:, idx].transpose(0, 1).float().unsqueeze(-1)
        return out
