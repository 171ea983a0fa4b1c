"""The replay rings of the three collectors, on the device: ``TransitionReplay`` (IDQ, one row per
agent), ``JointReplay`` (map-QMIX, one joint row per env) -- both with the cursor on the device,
advanced by ``add`` without a host round trip -- and ``EpisodeReplay`` (QMIX, whole episodes in
plain torch ops, host cursor)."""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream_handle
from .actions import ACTION_DIM


def _shape(s):
    return (int(s),) if isinstance(s, int) else tuple(int(x) for x in s)


def _floats(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _draw(size, batch_size, generator, device):
    """``batch_size`` distinct indices below ``size`` (torch's ``randperm`` on the generator's
    device, not numpy's global stream); with fewer than that stored, all of them in ring order."""
    if size < int(batch_size):
        return torch.arange(size, device=device)
    gdev = generator.device if generator is not None else torch.device("cpu")
    return torch.randperm(size, generator=generator, device=gdev)[:int(batch_size)].to(device)


class _DeviceRing:
    """A ring of ``capacity`` rows whose cursor (ptr, size) is an int64 tensor [2] on the device."""

    def __init__(self, capacity: int, device):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError(f"{type(self).__name__}: capacity must be >= 1")
        self.device = torch.device(device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)

    def position(self):
        """(ptr, size) read from the device: one 16-byte copy and a synchronisation."""
        p, s = self.cursor.tolist()
        return int(p), int(s)

    def __len__(self):
        """The number of stored rows.  Reads the device cursor (``position``): it synchronises."""
        return self.position()[1]

    def can_sample(self, batch_size: int) -> bool:
        return len(self) >= int(batch_size)

    def _draw(self, batch_size, generator):
        return _draw(len(self), batch_size, generator, self.device)

    def _check(self, who, want):
        """want: {name: (tensor, dtype, entries)} of ``add``'s arguments."""
        for name, (t, dt, n) in want.items():
            if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or t.device != self.cursor.device:
                raise TypeError(f"{who}: {name} must be a contiguous {dt} tensor on {self.cursor.device}")
            if t.numel() != n:
                raise ValueError(f"{who}: {name} holds {t.numel()} entries, needs {n}")


class TransitionReplay(_DeviceRing):
    """The reference's per-transition ``ReplayBuffer`` (IDQ/networks.py:46-104) as a device ring:
    observations / next_observations float32 [capacity, *obs_shape], actions int64, rewards
    float32, dones uint8 [capacity], and the cursor (ptr, size) as an int64 tensor [2] on the
    device, advanced by ``add`` without a host round trip."""

    def __init__(self, capacity: int, obs_shape, device="cuda"):
        super().__init__(capacity, device)
        self.obs_shape = _shape(obs_shape)
        self.row_floats = _floats(self.obs_shape)
        f = dict(dtype=torch.float32, device=self.device)
        self.observations = torch.zeros((self.capacity,) + self.obs_shape, **f)
        self.next_observations = torch.zeros((self.capacity,) + self.obs_shape, **f)
        self.actions = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self.rewards = torch.zeros(self.capacity, **f)
        self.dones = torch.zeros(self.capacity, dtype=torch.uint8, device=self.device)
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
        self._check("TransitionReplay.add", dict(
            filled=(filled, torch.uint8, E), done=(done, torch.uint8, E), actions=(actions, torch.uint8, E * A),
            reward=(reward, torch.float64, E * A), obs=(obs, torch.float32, E * A * self.row_floats),
            next_obs=(next_obs, torch.float32, E * A * self.row_floats)))
        if self._rank is None or self._rank.numel() < E + 3:
            self._rank = torch.zeros(E + 3, dtype=torch.int32, device=self.cursor.device)
        check(lib().mdl_replay_append(ptr(filled), E, A, self.row_floats, ptr(obs), ptr(next_obs), ptr(actions),
                                      ptr(reward), ptr(done), self.capacity, ptr(self.cursor), ptr(self.observations),
                                      ptr(self.next_observations), ptr(self.actions), ptr(self.rewards),
                                      ptr(self.dones), ptr(self._rank), stream_handle(self.cursor.device)),
              "mdl_replay_append")

    def sample(self, batch_size: int, generator=None):
        """``ReplayBuffer.sample`` (IDQ/networks.py:81-104): ``batch_size`` distinct stored rows as
        (obs float32, actions int64, rewards float32, next_obs float32, dones float32); with
        fewer than ``batch_size`` rows stored, all of them in ring order.  Reads the device cursor
        (one 16-byte copy and a synchronisation): sampling sits on the learner's side of the
        loop.  The draw is torch's ``randperm`` (``generator``), not numpy's global stream."""
        idx = self._draw(batch_size, generator)
        return (self.observations[idx], self.actions[idx], self.rewards[idx], self.next_observations[idx],
                self.dones[idx].float())


class JointReplay(_DeviceRing):
    """The ``qmix/`` trainer's joint ``ReplayBuffer`` (qmix/networks.py:155-239) as a device ring,
    its tensors named and shaped as the reference's arrays: states / next_states float32
    [capacity, *state_shape], observations / next_observations float32 [capacity, A, *obs_shape],
    actions int64 [capacity, A], total_reward float32 [capacity, 1], dones uint8 [capacity, 1], and
    the cursor (ptr, size) as an int64 tensor [2] on the device, advanced by ``add`` without a host
    round trip."""

    def __init__(self, capacity: int, n_agents: int, obs_shape, state_shape, device="cuda"):
        super().__init__(capacity, device)
        self.n_agents = int(n_agents)
        if self.n_agents < 1:
            raise ValueError("JointReplay: n_agents must be >= 1")
        self.obs_shape, self.state_shape = _shape(obs_shape), _shape(state_shape)
        self.obs_floats, self.state_floats = _floats(self.obs_shape), _floats(self.state_shape)
        f = dict(dtype=torch.float32, device=self.device)
        cap, A = self.capacity, self.n_agents
        self.states = torch.zeros((cap,) + self.state_shape, **f)
        self.next_states = torch.zeros((cap,) + self.state_shape, **f)
        self.observations = torch.zeros((cap, A) + self.obs_shape, **f)
        self.next_observations = torch.zeros((cap, A) + self.obs_shape, **f)
        self.actions = torch.zeros((cap, A), dtype=torch.int64, device=self.device)
        self.total_reward = torch.zeros((cap, 1), **f)
        self.dones = torch.zeros((cap, 1), dtype=torch.uint8, device=self.device)

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
        self._check("JointReplay.add", dict(
            state=(state, torch.float32, E * self.state_floats),
            next_state=(next_state, torch.float32, E * self.state_floats),
            obs=(obs, torch.float32, E * A * self.obs_floats), next_obs=(next_obs, torch.float32, E * A * self.obs_floats),
            actions=(actions, torch.uint8, E * A), reward=(reward, torch.float64, E), done=(done, torch.uint8, E)))
        check(lib().mdl_replay_append_joint(E, A, self.state_floats, self.obs_floats, ptr(state), ptr(next_state),
                                            ptr(obs), ptr(next_obs), ptr(actions), ptr(reward), ptr(done),
                                            self.capacity, ptr(self.cursor), ptr(self.states), ptr(self.next_states),
                                            ptr(self.observations), ptr(self.next_observations), ptr(self.actions),
                                            ptr(self.total_reward), ptr(self.dones),
                                            stream_handle(self.cursor.device)), "mdl_replay_append_joint")

    def sample(self, batch_size: int, generator=None):
        """``ReplayBuffer.sample`` (qmix/networks.py:200-235): ``batch_size`` distinct stored rows as
        the reference's tuple in the reference's order, (states, next_states, obs, next_obs,
        actions int64, total_rewards float32 [B, 1], dones float32 [B, 1]); with fewer than
        ``batch_size`` rows stored, all of them in ring order; an empty ring gives empty tensors.
        Reads the device cursor (a synchronisation): sampling sits on the learner's side of the
        loop.  The draw is torch's ``randperm`` (``generator``), not numpy's global stream."""
        idx = self._draw(batch_size, generator)
        return (self.states[idx], self.next_states[idx], self.observations[idx], self.next_observations[idx],
                self.actions[idx], self.total_reward[idx], self.dones[idx].float())


class EpisodeReplay:
    """The reference's episode ``ReplayBuffer`` (QMIX/networks.py:209-318) as a time-major ring
    of ``capacity`` episodes in plain torch ops, on the device of the template's tensors.

    ``collector``: a ``QmixCollector`` or one of its batches (a dict with so, vo, gs, gv, u, r,
    terminated, filled) -- the template for shapes, dtypes and device.  A template with an
    ``avail`` field (uint8 [L+1, E, A, n_actions], ``QmixCollector(avail=True)``) makes the ring
    store the valid-action masks too (``self.fields``; ``FIELDS`` is the reference's set).  A window-form
    template (``QmixCollector(ego_radius=R, ego_dtype=...)``) gives a ring whose so is
    [L+1, capacity, A, 6, K, K] of that dtype, and ``sample`` returns so / so_next [B, L, A, 6, K, K] in
    it: nothing here depends on the map's shape or on float32.

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
        self.fields = self.FIELDS + (("avail",) if tpl.get("avail") is not None else ())
        self.buf = {}
        for k in self.fields:
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
        for k in self.fields:
            self.buf[k][:, slots] = batch[k][:, first:]
        self.idx = (self.idx + E) % self.capacity
        self.size = min(self.capacity, self.size + E)

    def sample(self, batch_size: int, generator=None):
        """``batch_size`` distinct stored episodes as the reference's dictionary
        (QMIX/networks.py:299-314), episode-major: so / vo / gs / gv and their ``_next`` forms
        ([B, L, ...]; ``*_next`` is the same gathered tensor shifted by one slot, not a second
        copy), u int64 [B, L, A, 1], r [B, L, 1], avail_u / avail_u_next float32 [B, L, A,
        n_actions] (the stored masks of slots 0..L-1 and 1..L, two views of one gather, when the
        ring stores ``avail``; otherwise all ones, as QMIX/trainer.py:395-397 fills them),
        terminated and padded (= 1 - filled) float32 [B, L, 1]."""
        B = int(batch_size)
        if B < 1 or self.size < B:
            raise ValueError(f"EpisodeReplay holds {self.size} episodes, cannot sample {B}")
        idx = _draw(self.size, B, generator, self.device)
        L = self.L
        out = {}
        for k in ("so", "vo", "gs", "gv"):
            x = self.buf[k][:, idx].transpose(0, 1)   # [B, L+1, ...]
            out[k] = x[:, :L]
            out[k + "_next"] = x[:, 1:]
        A = self.buf["u"].shape[2]
        out["u"] = self.buf["u"][:, idx].transpose(0, 1).long().unsqueeze(-1)
        out["r"] = self.buf["r"][:, idx].transpose(0, 1).unsqueeze(-1)
        if "avail" in self.buf:
            av = self.buf["avail"][:, idx].transpose(0, 1).float()   # [B, L+1, A, n_actions]
            out["avail_u"] = av[:, :L]
            out["avail_u_next"] = av[:, 1:]
        else:
            ones = torch.ones((), dtype=torch.float32, device=self.device).expand(B, L, A, self.n_actions)
            out["avail_u"] = ones
            out["avail_u_next"] = ones
        out["terminated"] = self.buf["terminated"][:, idx].transpose(0, 1).float().unsqueeze(-1)
        out["padded"] = 1.0 - self.buf["filled"][:, idx].transpose(0, 1).float().unsqueeze(-1)
        return out
