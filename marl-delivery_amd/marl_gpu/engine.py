"""Tensor API of the MI355X batched step engine.

``BatchedEnv`` holds E independent marl-delivery environments resident in HBM
and steps them with one gfx950 kernel launch per step (one wavefront per env).
It is the batched counterpart of ``VectorizedEnv(Environment, E, ...)``
(MAPPO/env_vectorized.py:1-24, QMIX/env_vectorized.py:1-49) fused with the
MAPPO rollout glue that surrounds it (MAPPO/trainer.py:194-286): integer
action decode, ``compute_shaped_rewards`` with the pre-step tracker, the
persistent-package tracker update and reset-on-done all run on the device.

Inputs and outputs are torch tensors on the engine's device; every call is
asynchronous on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_handle
from ._lib import raw_stream as _raw_stream
from .actions import ACTION_DIM
from .maps import grid_array, load_map, map_path

# shaping constants, order: pickup, on_time, late, closer, wasted_pick,
# wasted_drop, stuck, idle, away  (MAPPO/helper.py:271-279, QMIX/helper.py:270-278)
MAPPO_SHAPING = (5, 200, 20, 0.02, 0, 0, -0.05, -0.05, -0.01)
QMIX_SHAPING = (0.5, 2.0, 0.2, 0.02, -0.1, -0.1, -0.05, -0.02, -0.02)

TRACKER_MODES = {"fresh": _lib.MDL_TRACKER_FRESH, "mappo": _lib.MDL_TRACKER_MAPPO_STALE,
                 "mappo_stale": _lib.MDL_TRACKER_MAPPO_STALE}
ACTION_FORMATS = {"int": _lib.MDL_ACTION_TRAINER_INT, "codes": _lib.MDL_ACTION_CODES}
OBS_BUILDERS = {"auto": _lib.MDL_OBS_BUILDER_AUTO, "generic": _lib.MDL_OBS_BUILDER_GENERIC}
STEP_LAYOUTS = {"auto": _lib.MDL_STEP_LAYOUT_AUTO, "wave": _lib.MDL_STEP_LAYOUT_WAVE, "rows": _lib.MDL_STEP_LAYOUT_ROWS,
                "halves": _lib.MDL_STEP_LAYOUT_HALVES}
_LAYOUT_NAMES = {_lib.MDL_STEP_LAYOUT_WAVE: "wave", _lib.MDL_STEP_LAYOUT_ROWS: "rows", _lib.MDL_STEP_LAYOUT_HALVES: "halves"}
STATUS_NAMES = ("None", "waiting", "in_transit", "delivered")
OBS_KEYS = ("actor_map", "actor_vec", "critic_map", "critic_vec")
# element types of the MAPPO/QMIX observation tensors (build_obs / step_obs): float32, or the float32
# value rounded once to nearest-even (bit for bit ``x.to(dtype)``)
OBS_DTYPES = {torch.float32: _lib.MDL_OBS_F32, torch.float16: _lib.MDL_OBS_F16, torch.bfloat16: _lib.MDL_OBS_BF16}
ALT_KEYS = ("idq_obs", "qmix_state")


def _obs_dtype(dtype):
    if dtype not in OBS_DTYPES:
        raise TypeError(f"observation dtype must be torch.float32, torch.float16 or torch.bfloat16, not {dtype}")
    return OBS_DTYPES[dtype]


def _as_grid(m):
    if isinstance(m, str):
        return grid_array(load_map(map_path(m)))
    return grid_array(m)


class BatchedEnv:
    """E environments on one GPU.

    maps:      one map (path / name / 2-D 0-1 array) or a list of up to 8 maps;
    env_map:   per-env map index when several maps are given (contiguous
               groups keep each observation tensor single-shaped);
    seeds:     per-env RandomState seeds; default ``seed + i`` like
               VectorizedEnv (MAPPO/env_vectorized.py:8-9);
    tracker:   "mappo" (never cleared on auto-reset, MAPPO/trainer.py:232-233)
               or "fresh" (== env truth, QMIX/evaluation semantics);
    shaping:   "mappo" | "qmix" | 9 constants;
    obs dims:  max_other_robots / max_packages_obs (generate_vector_features),
               max_robots_state / max_packages_state (convert_global_state);
               obs_max_time_steps defaults to max_time_steps;
    obs_builder:   "auto" (the small builder where it applies, A <= 8 and P <= 64) or
               "generic" (always the general builder): the same observations either way.
    step_layout:   "auto" (four envs per wavefront for full-batch steps of >= 7,168 envs where A <= 8
               and P <= 64; two for >= 12,288 envs where A == 16 and P <= 128), "wave" (one env per
               wavefront), "rows" (four per wavefront) or "halves" (two per wavefront; both an error
               where they do not apply): the same results either way (MdlConfig.step_layout).
    After construction every env holds the constructor's layout draw; call
    ``reset()`` for the first episode, as the reference trainers do.
    """

    def __init__(self, maps, n_envs: int, n_robots: int = 5, n_packages: int = 20, max_time_steps: int = 100,
                 move_cost: float = -0.01, delivery_reward: float = 10.0, delay_reward: float = 1.0,
                 seed: int = 2025, seeds: Sequence[int] | None = None, env_map: Sequence[int] | None = None,
                 tracker: str = "mappo", shaping="mappo", max_other_robots: int | None = None,
                 max_packages_obs: int = 5, max_robots_state: int = 100, max_packages_state: int = 100,
                 obs_max_time_steps: int | None = None, obs_builder: str = "auto", step_layout: str = "auto",
                 device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("marl_gpu.BatchedEnv needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"marl_gpu.BatchedEnv runs on a GPU device, not {self.device}")
        if self.device.index is None:   # "cuda" -> the current device, explicitly
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(maps, (str, np.ndarray)) or (isinstance(maps, list) and maps and isinstance(maps[0], list)
                                                  and maps[0] and isinstance(maps[0][0], (int, np.integer))):
            maps = [maps]
        self.grids = [_as_grid(m) for m in maps]
        self.E, self.A, self.P, self.T = int(n_envs), int(n_robots), int(n_packages), int(max_time_steps)
        if isinstance(shaping, str):
            shaping = {"mappo": MAPPO_SHAPING, "qmix": QMIX_SHAPING}[shaping]
        self.shaping = tuple(float(x) for x in shaping)
        self.tracker = tracker
        self.MO = self.A - 1 if max_other_robots is None else int(max_other_robots)
        self.MP, self.MR, self.MPs = int(max_packages_obs), int(max_robots_state), int(max_packages_state)
        self.obs_T = self.T if obs_max_time_steps is None else int(obs_max_time_steps)
        cfg = _lib.MdlConfig()
        cfg.n_envs, cfg.n_robots, cfg.n_packages, cfg.max_time_steps = self.E, self.A, self.P, self.T
        cfg.move_cost, cfg.delivery_reward, cfg.delay_reward = float(move_cost), float(delivery_reward), float(delay_reward)
        cfg.tracker_mode = TRACKER_MODES[tracker]
        for i, v in enumerate(self.shaping):
            cfg.shaping[i] = v
        cfg.obs_max_time_steps = self.obs_T
        cfg.max_other_robots, cfg.max_packages_obs = self.MO, self.MP
        cfg.max_robots_state, cfg.max_packages_state = self.MR, self.MPs
        cfg.obs_builder = OBS_BUILDERS[obs_builder]
        cfg.step_layout = STEP_LAYOUTS[step_layout]
        self.cfg = cfg
        flat = np.ascontiguousarray(np.concatenate([g.reshape(-1) for g in self.grids]).astype(np.uint8))
        hw = np.array([[g.shape[0], g.shape[1]] for g in self.grids], np.int32).reshape(-1)
        if env_map is None:
            env_map = [0] * self.E if len(self.grids) == 1 else None
            if env_map is None:
                raise ValueError("env_map is required with several maps")
        self.env_map = np.ascontiguousarray(np.asarray(env_map, np.int32))
        if self.env_map.shape != (self.E,):
            raise ValueError("env_map must have one entry per env")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mdl_create(C.byref(cfg), flat.ctypes.data, hw.ctypes.data, len(self.grids),
                                   self.env_map.ctypes.data, self.device.index, C.byref(h)), "mdl_create")
        self._h = h
        av, cv = C.c_int32(), C.c_int32()
        check(lib().mdl_obs_dims(self._h, C.byref(av), C.byref(cv)))
        self.actor_vec_dim, self.critic_vec_dim = av.value, cv.value
        # whether a full-batch step runs four envs per wavefront: the engine's own decision
        self.step_rows = self.step_layout() == "rows"
        if seeds is None:
            seeds = [int(seed) + i for i in range(self.E)]
        self.seeds = np.ascontiguousarray(np.asarray(seeds, np.int64) & 0xFFFFFFFF).astype(np.uint32)
        if self.seeds.shape != (self.E,):
            raise ValueError("seeds must have one entry per env")
        with torch.cuda.device(self.device):
            check(lib().mdl_seed(self._h, self.seeds.ctypes.data, C.c_void_p(stream_handle(self.device))),
                  "mdl_seed")
        # reusable outputs
        self._r = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        self._sh = torch.zeros(self.E, dtype=torch.float32, device=self.device)
        self._done = torch.zeros(self.E, dtype=torch.uint8, device=self.device)
        self._fn_step = lib().mdl_step
        self._out_ok = None
        self._dev = self.device.index
        self._full_out = (self._r, self._sh, self._done)
        # end (exclusive) of each env's run of consecutive envs with the same map shape:
        # an observation range must lie inside one run (its tensors have one H x W)
        hw_env = np.array([self.grids[m].shape for m in self.env_map], np.int64).reshape(self.E, 2)
        brk = np.nonzero(np.any(hw_env[1:] != hw_env[:-1], axis=1))[0] + 1
        ends = np.append(brk, self.E)
        self._shape_run_end = np.repeat(ends, np.diff(np.concatenate(([0], ends))))

    def single_map_shape(self, who: str):
        """(H, W) of the one map shape all envs share; ValueError (``who`` names the caller, whose
        buffers hold one [H, W]) if the envs mix shapes."""
        if self._shape_run_end[0] < self.E:
            raise ValueError(f"{who}: the engine's envs mix map shapes (build one engine per map shape)")
        H, W = self.grids[int(self.env_map[0])].shape
        return int(H), int(W)

    # ------------------------------------------------------------------ core
    def close(self):
        if getattr(self, "_h", None):
            # the mailbox context (compat's C step path) holds raw engine addresses: drop it first
            self.__dict__.pop("_mail_ctx", None)
            self.__dict__.pop("_mb", None)
            lib().mdl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(stream_handle(self.device))

    def _ids(self, env_ids):
        """Env-id subset -> (int32 device tensor or None, count).

        Host-side ids (list / numpy / CPU tensor) are checked like the reference's
        ``self.envs[i]`` indexing: negatives count from the end, anything outside
        [-E, E) raises IndexError.  Duplicates raise ValueError (one launch steps
        every listed env once, in parallel; ``compat.VectorizedEnv`` splits repeated
        ids into sequential launches as the reference's loop does).  Device tensors
        are taken as they are, without a host round trip: their ids must be unique
        and in [0, E) (the kernels skip ids outside that range, so a bad id cannot
        touch another env's memory, but it is not reported)."""
        if env_ids is None:
            return None, self.E
        if isinstance(env_ids, torch.Tensor) and env_ids.is_cuda:
            ids = env_ids
            if ids.dtype != torch.int32 or ids.get_device() != self.device.index or not ids.is_contiguous():
                ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
            return ids.reshape(-1), int(ids.numel())
        a = np.asarray(env_ids.numpy() if isinstance(env_ids, torch.Tensor) else env_ids).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"env ids must be integers, got {a.dtype}")
        a = a.astype(np.int64)
        if a.size and (a.min() < -self.E or a.max() >= self.E):
            raise IndexError(f"env id out of range for {self.E} envs")
        a = np.where(a < 0, a + self.E, a)
        if np.unique(a).size != a.size:
            raise ValueError("duplicate env ids in one call (each listed env is stepped once, in parallel)")
        return torch.from_numpy(a.astype(np.int32)).to(self.device), int(a.size)

    def reset(self, env_ids=None):
        """Environment.reset() for all envs or a subset (QMIX/env_vectorized.py:13-21)."""
        ids, n = self._ids(env_ids)
        if n == 0:
            return
        check(lib().mdl_reset(self._h, ptr(ids), n, self._stream()), "mdl_reset")
        self._keep = ids

    def clear_tracker(self, env_ids=None):
        ids, n = self._ids(env_ids)
        if n == 0:
            return
        check(lib().mdl_tracker_clear(self._h, ptr(ids), n, self._stream()), "mdl_tracker_clear")
        self._keep = ids

    def _check_out(self, out, shape):
        """The caller's (r_env f64, r_shaped f32, done uint8) buffers: dtype, device, size.
        The last checked buffers are remembered (objects, shape, addresses), so a step loop
        that reuses its buffers pays for the full check once."""
        if len(out) != 3:
            raise ValueError("out must be (r_env, r_shaped, done)")
        want = 1
        for s in shape:
            want *= s
        for t, dt, name in zip(out, (torch.float64, torch.float32, torch.uint8), ("r_env", "r_shaped", "done")):
            self._check_vec(t, dt, f"out {name}", want)
        self._out_ok = (out[0], out[1], out[2], shape, (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()))

    def _out_ptrs(self, out, shape):
        """Addresses of checked output buffers (the full check only for new buffers)."""
        r, sh, d = out
        ptrs = (r.data_ptr(), sh.data_ptr(), d.data_ptr())
        m = self._out_ok
        if m is None or r is not m[0] or sh is not m[1] or d is not m[2] or m[3] != shape or m[4] != ptrs:
            self._check_out(out, shape)
        return ptrs

    def _step_args(self, actions, n, lead=()):
        if actions.dtype != torch.uint8 or not actions.is_cuda or actions.get_device() != self.device.index \
                or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.uint8).contiguous()
        if actions.numel() != n * self.A * (lead[0] if lead else 1) \
                or (lead and (actions.dim() != 3 or actions.shape[1] != n or actions.shape[2] != self.A)):
            raise ValueError(f"actions must be [{', '.join(str(x) for x in lead + (n, self.A))}]")
        return actions

    def step(self, actions: torch.Tensor, env_ids=None, auto_reset: bool = True, action_format: str = "int",
             out=None):
        """One transition for all envs (or ``env_ids``).

        actions: uint8 tensor [n, A] on the device -- trainer ints 0..14
        (MAPPO/trainer.py:198-205) or packed codes (action_format="codes").
        Returns (r_env f64 [n], r_shaped f32 [n], done uint8 [n]) views of
        reusable buffers unless ``out`` is given (then: float64 / float32 / uint8
        tensors of >= n entries on the engine's device).
        """
        if env_ids is None:
            ids, n = None, self.E
        else:
            ids, n = self._ids(env_ids)
        if actions.dtype is not torch.uint8 or not actions.is_cuda or not actions.is_contiguous() \
                or actions.get_device() != self._dev or actions.numel() != n * self.A:
            actions = self._step_args(actions, n)
        if out is None:
            out = self._full_out if n == self.E else (self._r[:n], self._sh[:n], self._done[:n])
            ptrs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        else:
            ptrs = self._out_ptrs(out, (n,))
        if n == 0:
            return out
        check(self._fn_step(self._h, actions.data_ptr(), ACTION_FORMATS[action_format],
                            None if ids is None else ids.data_ptr(), n, 1 if auto_reset else 0,
                            ptrs[0], ptrs[1], ptrs[2], _raw_stream(self._dev)), "mdl_step")
        self._keep = (ids, actions)
        return out[0], out[1], out[2]

    def step_obs(self, actions: torch.Tensor, auto_reset: bool = True, action_format: str = "int", out=None,
                 obs_out: dict | None = None, which=("actor_map", "actor_vec", "critic_map", "critic_vec"),
                 obs_dtype: torch.dtype = torch.float32):
        """``step`` over all envs, then ``build_obs`` of the new state (the trainer's per-step
        sequence, MAPPO/trainer.py:229-286), as one launch when A <= 8 and P <= 64: the
        kernel builds the observations from the state the step leaves in registers.
        Bit-identical to ``step(...)`` followed by ``build_obs()``.  The envs must share one
        map shape.  Returns (r_env, r_shaped, done, obs dict); without ``obs_out`` the obs
        tensors are the engine's own buffers, overwritten by the next call.

        ``obs_dtype``: the observation tensors' element type, as ``build_obs(dtype=)``.  With
        torch.float16 / torch.bfloat16 the call is always the step launch followed by the builder's
        (the fused kernel writes float32 only); rewards, done and the engine's state are the same."""
        dt = _obs_dtype(obs_dtype)
        n = self.E
        if actions.dtype is not torch.uint8 or not actions.is_cuda or not actions.is_contiguous() \
                or actions.get_device() != self._dev or actions.numel() != n * self.A:
            actions = self._step_args(actions, n)
        if out is None:
            out = self._full_out
            ptrs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        else:
            ptrs = self._out_ptrs(out, (n,))
        if self._shape_run_end[0] < n:
            raise ValueError("step_obs: the envs mix map shapes; use step() and build_obs() per same-shape group")
        H, W = self.grids[int(self.env_map[0])].shape
        obs_out, op = self._obs_out(obs_out, which, n, H, W, dtype=obs_dtype)
        if dt == _lib.MDL_OBS_F32:
            check(lib().mdl_step_obs(self._h, actions.data_ptr(), ACTION_FORMATS[action_format],
                                     1 if auto_reset else 0, ptrs[0], ptrs[1], ptrs[2], *op, _raw_stream(self._dev)),
                  "mdl_step_obs")
        else:
            check(lib().mdl_step_obs_as(self._h, actions.data_ptr(), ACTION_FORMATS[action_format],
                                        1 if auto_reset else 0, ptrs[0], ptrs[1], ptrs[2], dt, *op,
                                        _raw_stream(self._dev)), "mdl_step_obs_as")
        self._keep = (None, actions)
        # only the outputs written by this call (a cached dict's other entries would be stale)
        return out[0], out[1], out[2], {k: (v if k in which else None) for k, v in obs_out.items()}

    def _check_buf(self, t, dtype, need, bad, misplaced=None, short=None):
        """A caller's buffer: a contiguous ``dtype`` tensor on the engine's device with at least
        ``need`` entries (an int) or of exactly the shape ``need`` (a tuple).  What is raised is the
        call site's: ``bad`` = (exception class, message) for a wrong type or dtype and, unless the
        site words them apart, ``misplaced`` for a wrong device or layout and ``short`` for the size
        (its message may hold ``{n}``, the tensor's entry count)."""
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise bad[0](bad[1])
        if not t.is_cuda or t.get_device() != self.device.index or not t.is_contiguous():
            err = misplaced or bad
            raise err[0](err[1])
        if (tuple(t.shape) != need) if isinstance(need, tuple) else (t.numel() < need):
            err = short or bad
            raise err[0](err[1].format(n=t.numel()))

    def _check_vec(self, t, dtype, name, n=None):
        """``_check_buf`` for a vector of ``n`` (default E) entries -- masks, per-env results -- in
        the three wordings those share."""
        n = self.E if n is None else n
        self._check_buf(t, dtype, n, (TypeError, f"{name} must be a {dtype} tensor"),
                        (ValueError, f"{name} must be contiguous on {self.device}"),
                        (ValueError, f"{name} holds {{n}} entries, needs {n}"))

    def _check_mask(self, t, name):
        self._check_vec(t, torch.uint8, name)

    def step_episode(self, actions: torch.Tensor, active: torch.Tensor, action_format: str = "int", out=None,
                     filled: torch.Tensor | None = None, obs_out: dict | None = None,
                     which=("actor_map", "actor_vec", "critic_map", "critic_vec")):
        """One transition of an episode batch (QMIX/trainer.py:363-511 steps only the envs whose
        episode still runs): ``step(auto_reset=False)`` + ``build_obs`` for the envs whose byte of
        ``active`` (uint8 [E] on the device, the caller's) is set, with no host round trip -- one
        launch where ``step_obs`` is one.  A done env's byte is cleared on the device.  The other
        envs are not touched: their r_env / r_shaped / done / ``filled`` are 0 and their rows of
        ``obs_out`` are left unwritten.  Never resets.  Returns (r_env, r_shaped, done, obs dict);
        ``filled`` (uint8 [E]) receives 1 for the envs that were stepped.

        An engine whose envs mix map shapes takes ``which=()`` only (the step alone; the dict's entries
        are None): ``build_obs_canvas(rows=filled)`` and ``build_obs_ego_masked(filled)`` write the
        observations of such a batch.  With an observation named it raises, as on any mixed engine."""
        n = self.E
        if actions.dtype is not torch.uint8 or not actions.is_cuda or not actions.is_contiguous() \
                or actions.get_device() != self._dev or actions.numel() != n * self.A:
            actions = self._step_args(actions, n)
        self._check_mask(active, "active")
        if filled is not None:
            self._check_mask(filled, "filled")
        if out is None:
            out = self._full_out
            ptrs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        else:
            ptrs = self._out_ptrs(out, (n,))
        if not which and self._shape_run_end[0] < self.E:
            # mixed map shapes: the step alone (build_obs_canvas and the window builders follow it)
            obs_out, op = dict.fromkeys(OBS_KEYS), [None] * 4
        else:
            H, W = self.single_map_shape("step_episode")
            obs_out, op = self._obs_out(obs_out, which, n, H, W)
        check(lib().mdl_step_episode(self._h, actions.data_ptr(), ACTION_FORMATS[action_format], active.data_ptr(),
                                     ptrs[0], ptrs[1], ptrs[2], ptr(filled), *op, _raw_stream(self._dev)),
              "mdl_step_episode")
        self._keep = (None, actions)
        return out[0], out[1], out[2], {k: (v if k in which else None) for k, v in obs_out.items()}

    def step_fused(self, actions: torch.Tensor, env_ids=None, auto_reset: bool = True, action_format: str = "int",
                   out=None):
        """Bench mode: K consecutive steps in one launch.

        actions: uint8 [K, n, A]; returns (r_env f64 [K, n], r_shaped f32 [K, n],
        done uint8 [K, n]), identical to K ``step`` calls with actions[k].
        """
        ids, n = self._ids(env_ids)
        if actions.dim() != 3:
            raise ValueError(f"actions must be [K, {n}, {self.A}]")
        K = actions.shape[0]
        actions = self._step_args(actions, n, (K,))
        if out is None:
            r = torch.empty((K, n), dtype=torch.float64, device=self.device)
            sh = torch.empty((K, n), dtype=torch.float32, device=self.device)
            d = torch.empty((K, n), dtype=torch.uint8, device=self.device)
        else:
            self._out_ptrs(out, (K, n))
            r, sh, d = out
        if n == 0 or K == 0:
            return r, sh, d
        check(lib().mdl_step_fused(self._h, ptr(actions), ACTION_FORMATS[action_format], ptr(ids), n, K,
                                   int(bool(auto_reset)), ptr(r), ptr(sh), ptr(d), self._stream()), "mdl_step_fused")
        self._keep = (ids, actions)
        return r, sh, d

    def step_layout(self, n: int | None = None) -> str:
        """The layout ``step`` launches ("wave": one env per wavefront, "rows": four, "halves": two) for the full
        batch (n None) or an ``env_ids`` subset of n envs -- asked of the engine (mdl_step_layout),
        which takes the same decision inside mdl_step."""
        lay = C.c_int32()
        check(lib().mdl_step_layout(self._h, self.E if n is None else int(n), 0 if n is None else 1,
                                    C.byref(lay)), "mdl_step_layout")
        return _LAYOUT_NAMES[lay.value]

    def step_kernel_name(self, layout: str | None = None, with_obs: bool = False) -> str:
        """The kernel symbol (as rocprof names it) ``step`` launches in ``layout`` (default: the
        full batch's), or ``step_obs``'s step launch with ``with_obs`` -- from the engine."""
        lay = ("wave" if with_obs else self.step_layout()) if layout is None else layout
        buf = C.create_string_buffer(128)
        check(lib().mdl_step_kernel_name(self._h, STEP_LAYOUTS[lay], 1 if with_obs else 0, buf, 128),
              "mdl_step_kernel_name")
        return buf.value.decode()

    def obs_kernel_name(self, dtype: torch.dtype = torch.float32) -> str:
        """The kernel symbol (as rocprof names it) ``build_obs(dtype=dtype)`` launches -- from the
        engine, whose builder launch goes through the same selection."""
        buf = C.create_string_buffer(128)
        check(lib().mdl_obs_kernel_name(self._h, _obs_dtype(dtype), buf, 128), "mdl_obs_kernel_name")
        return buf.value.decode()

    def last_step_layout(self) -> str | None:
        """The layout of the last ``step`` launch (None before the first), as the engine recorded it."""
        lay = C.c_int32()
        check(lib().mdl_last_step_layout(self._h, C.byref(lay)), "mdl_last_step_layout")
        return None if lay.value == 0 else _LAYOUT_NAMES[lay.value]

    def step_floor(self, n: int | None = None):
        """Measurement aid: one launch of an empty kernel in ``step``'s launch shape over n envs
        (grid, workgroup, LDS, kernel arguments); touches no state.  bench.py's launch floor."""
        n = self.E if n is None else int(n)
        check(lib().mdl_step_floor(self._h, n, _raw_stream(self._dev)), "mdl_step_floor")

    def obs_buffers(self, n=None, H=None, W=None, dtype: torch.dtype = torch.float32):
        """New observation tensors for n envs of an [H, W] map, of element type ``dtype``
        (torch.float32, torch.float16 or torch.bfloat16: what ``build_obs`` / ``step_obs`` write)."""
        _obs_dtype(dtype)
        n = self.E if n is None else n
        H = self.grids[0].shape[0] if H is None else H
        W = self.grids[0].shape[1] if W is None else W
        f = dict(dtype=dtype, device=self.device)
        return dict(actor_map=torch.empty((n, self.A, 6, H, W), **f),
                    actor_vec=torch.empty((n, self.A, self.actor_vec_dim), **f),
                    critic_map=torch.empty((n, 4, H, W), **f),
                    critic_vec=torch.empty((n, self.critic_vec_dim), **f))

    def _obs_range(self, env_begin, n):
        """Checked env range of one observation call -> (n, grid of its map shape)."""
        env_begin = int(env_begin)
        n = self.E - env_begin if n is None else int(n)
        if env_begin < 0 or n < 0 or env_begin + n > self.E:
            raise IndexError(f"env range [{env_begin}, {env_begin + n}) outside [0, {self.E})")
        if n == 0:
            return n, self.grids[0]
        if self._shape_run_end[env_begin] < env_begin + n:
            raise ValueError(f"envs [{env_begin}, {env_begin + n}) mix map shapes: build observations per "
                             f"same-shape group (this one ends at env {int(self._shape_run_end[env_begin])})")
        return n, self.grids[int(self.env_map[env_begin])]

    def _check_obs_out(self, t, name, shape, dtype=torch.float32):
        want = 1
        for s in shape:
            want *= s
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} device tensor")
        if t.get_device() != self.device.index:
            raise ValueError(f"{name} must be on {self.device}, not cuda:{t.get_device()}")
        if t.numel() < want:
            raise ValueError(f"{name} holds {t.numel()} floats, needs {want} {tuple(shape)}")

    def _obs_out(self, obs_out, which, n, H, W, strict=False, dtype=torch.float32):
        """The observation outputs of one call over n envs of an [H, W] map -> (the dict, the four
        addresses in ``OBS_KEYS`` order).  Without ``obs_out`` the engine's own cached buffers (one set
        per ``dtype``).  Only the entries ``which`` names are written (the others: address None), each
        checked against its shape and ``dtype``; ``strict``: a named entry must be in the dict."""
        if obs_out is None:
            cache = getattr(self, "_obs_cache", None)
            if cache is None:
                cache = self._obs_cache = {}
            obs_out = cache.get(dtype)
            if obs_out is None:
                obs_out = cache[dtype] = self.obs_buffers(n, H, W, dtype)
        shapes = dict(actor_map=(n, self.A, 6, H, W), actor_vec=(n, self.A, self.actor_vec_dim),
                      critic_map=(n, 4, H, W), critic_vec=(n, self.critic_vec_dim))
        op = []
        for k in OBS_KEYS:
            t = (obs_out[k] if strict else obs_out.get(k)) if k in which else None
            if t is not None:
                self._check_obs_out(t, k, shapes[k], dtype)
            op.append(ptr(t))
        return obs_out, op

    def _alt_out(self, out, n, H, W, state_shape, new=(), which=ALT_KEYS):
        """The IDQ / qmix outputs of one call over n envs of an [H, W] map -> (the dict, the idq_obs and
        qmix_state addresses, then oh, ow of the qmix state: ``state_shape`` (7, h, w) or the map's).
        Without ``out``, new tensors for the entries ``new`` names.  The entries present among those
        ``which`` names are checked against their shapes and written (the others: address None)."""
        oh, ow = (H, W) if state_shape is None else (int(state_shape[1]), int(state_shape[2]))
        shapes = dict(idq_obs=(n, self.A, 6, H, W), qmix_state=(n, 7, oh, ow))
        if out is None:
            out = {k: torch.empty(shapes[k], dtype=torch.float32, device=self.device) for k in ALT_KEYS if k in new}
        op = []
        for k in ALT_KEYS:
            t = out.get(k) if k in which else None
            if t is not None:
                self._check_obs_out(t, k, shapes[k])
            op.append(ptr(t))
        return out, op + [oh, ow]

    def build_obs(self, env_begin: int = 0, n: int | None = None, out: dict | None = None,
                  which=("actor_map", "actor_vec", "critic_map", "critic_vec"),
                  dtype: torch.dtype = torch.float32):
        """convert_observation / generate_vector_features / convert_global_state
        for every agent of envs [env_begin, env_begin+n) (one map shape: raises
        on a range that mixes map shapes).

        ``dtype``: the tensors' element type.  torch.float16 / torch.bfloat16 tensors hold the float32
        values rounded once to nearest-even -- bit for bit ``build_obs()[k].to(dtype)`` -- written as
        half elements by the builder itself (half the bytes: for a policy under autocast, or smaller
        rollout buffers).  ``out`` tensors must have that dtype.  (``step_episode``, the evaluator's and
        the QMIX collectors' full-map paths and the IDQ / qmix featurizers stay float32; their window forms
        take ``ego_dtype`` for the windows alone.)"""
        dt = _obs_dtype(dtype)
        n, g = self._obs_range(env_begin, n)
        H, W = g.shape
        out, op = self._obs_out(self.obs_buffers(n, H, W, dtype) if out is None else out, which, n, H, W,
                                strict=True, dtype=dtype)
        if n == 0:
            return out
        if dt == _lib.MDL_OBS_F32:
            check(lib().mdl_build_obs(self._h, env_begin, n, *op, self._stream()), "mdl_build_obs")
        else:
            check(lib().mdl_build_obs_as(self._h, env_begin, n, dt, *op, self._stream()), "mdl_build_obs_as")
        return out

    # ---- robot-centred actor-map windows ----
    @staticmethod
    def _ego_radius(radius):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) \
                or not 1 <= int(radius) <= _lib.MDL_EGO_MAX_RADIUS:
            raise ValueError(f"radius must be an int in [1, {_lib.MDL_EGO_MAX_RADIUS}], not {radius!r}")
        return int(radius)

    def ego_buffers(self, radius: int, n=None, dtype: torch.dtype = torch.float32):
        """A new tensor [n, A, 6, K, K] (K = 2 * radius + 1) of ``dtype`` for ``build_obs_ego``."""
        _obs_dtype(dtype)
        K = 2 * self._ego_radius(radius) + 1
        n = self.E if n is None else int(n)
        return torch.empty((n, self.A, 6, K, K), dtype=dtype, device=self.device)

    def build_obs_ego(self, radius: int, env_begin: int = 0, n: int | None = None, out: torch.Tensor | None = None,
                      dtype: torch.dtype = torch.float32):
        """Each robot's ``K x K`` window of its actor map, centred on the robot (K = 2 * radius + 1,
        radius in 1..15), for envs [env_begin, env_begin + n): a tensor [n, A, 6, K, K].

        ``ego[e, a, ch, i, j] = build_obs()["actor_map"][e, a, ch, r - radius + i, c - radius + j]`` for
        robot a on cell (r, c) where that cell lies inside the map -- same tracker mode, stale survivors
        and clock.  Outside the map channel 0 (obstacles) is 1.0 (an off-map cell cannot be entered) and
        channels 1-5 are 0.0, so channel 1 is a single 1.0 at (radius, radius) and the reference's actor
        constructs unchanged with ``obs_shape = (6, K, K)``.  The carried package's target (channel 5)
        may fall outside the window -- that is what a window means; channel 5 is then all zero while
        the robot carries, and the actor vector still holds the target.

        The shape does not depend on the map, so the range may cross map shapes (``build_obs`` refuses
        that).  ``dtype`` as ``build_obs``: the half types hold 0 / 1.0 exactly.  ``out``: a contiguous
        tensor of ``dtype`` on the engine's device with n * A * 6 * K * K entries.
        ``build_obs_ego_masked`` is the form under a device mask of envs."""
        return self._build_obs_ego(radius, env_begin, n, out, dtype, None)

    def build_obs_ego_masked(self, radius: int, rows: torch.Tensor, env_begin: int = 0, n: int | None = None,
                             out: torch.Tensor | None = None, dtype: torch.dtype = torch.float32):
        """``build_obs_ego`` for the envs of [env_begin, env_begin + n) that ``rows`` marks, for the
        episode loops (``rows`` = ``step_episode``'s ``filled``).  ``rows``: uint8 [E] on the engine's
        device, indexed by env id whatever the range; a non-zero byte = build.  The launch reads the
        mask itself (no host round trip, so the call can be captured in a hipGraph).  The output row of
        an env is where ``build_obs_ego`` puts it; the rows of unmarked envs are not written -- in a
        caller's ``out`` they keep what they held, and a fresh tensor (``out=None``) starts as zeros."""
        self._check_mask(rows, "rows")
        return self._build_obs_ego(radius, env_begin, n, out, dtype, rows)

    def _build_obs_ego(self, radius, env_begin, n, out, dtype, rows):
        dt = _obs_dtype(dtype)
        R = self._ego_radius(radius)
        K = 2 * R + 1
        env_begin = int(env_begin)
        n = self.E - env_begin if n is None else int(n)
        if env_begin < 0 or n < 0 or env_begin + n > self.E:
            raise IndexError(f"env range [{env_begin}, {env_begin + n}) outside [0, {self.E})")
        need = n * self.A * 6 * K * K
        if out is None:
            out = self.ego_buffers(R, n, dtype) if rows is None else \
                torch.zeros((n, self.A, 6, K, K), dtype=dtype, device=self.device)
        else:
            name = str(dtype).replace("torch.", "")
            self._check_buf(out, dtype, need, (TypeError, f"out must be a {name} tensor"),
                            (ValueError, f"out must be contiguous on {self.device}"),
                            (ValueError, f"out holds {{n}} entries, needs {need} ({n}, {self.A}, 6, {K}, {K})"))
        if n == 0:
            return out
        if rows is None:
            check(lib().mdl_build_obs_ego(self._h, env_begin, n, R, dt, ptr(out), self._stream()), "mdl_build_obs_ego")
        else:
            check(lib().mdl_build_obs_ego_masked(self._h, env_begin, n, ptr(rows), R, dt, ptr(out), self._stream()),
                  "mdl_build_obs_ego_masked")
        return out

    # ---- the critic map on a fixed canvas: observations of envs of several map shapes ----
    CANVAS_KEYS = ("actor_vec", "critic_map", "critic_vec")

    def _canvas(self, canvas):
        try:
            Hc, Wc = canvas
            ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (Hc, Wc))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"canvas must be a pair of ints (Hc, Wc), not {canvas!r}")
        Hc, Wc = int(Hc), int(Wc)
        if not (1 <= Hc <= 255 and 1 <= Wc <= 255 and Hc * Wc <= _lib.MDL_MAX_CELLS):
            raise ValueError(f"canvas {Hc} x {Wc}: Hc, Wc must be in [1, 255] with Hc * Wc <= {_lib.MDL_MAX_CELLS}")
        return Hc, Wc

    def canvas_buffers(self, canvas, n=None, dtype: torch.dtype = torch.float32):
        """New tensors of ``dtype`` for ``build_obs_canvas``: actor_vec [n, A, Dv], critic_map
        [n, 4, Hc, Wc] and critic_vec [n, Dg] for ``canvas = (Hc, Wc)``."""
        _obs_dtype(dtype)
        Hc, Wc = self._canvas(canvas)
        n = self.E if n is None else int(n)
        f = dict(dtype=dtype, device=self.device)
        return dict(actor_vec=torch.empty((n, self.A, self.actor_vec_dim), **f),
                    critic_map=torch.empty((n, 4, Hc, Wc), **f),
                    critic_vec=torch.empty((n, self.critic_vec_dim), **f))

    def build_obs_canvas(self, canvas, env_begin: int = 0, n: int | None = None, rows: torch.Tensor | None = None,
                         out: dict | None = None, which=("actor_vec", "critic_map", "critic_vec"),
                         dtype: torch.dtype = torch.float32):
        """The critic's observations of envs [env_begin, env_begin + n) of any map shapes: the critic map
        on the fixed canvas ``canvas = (Hc, Wc)`` and the two vector observations -> a dict.

        ``critic_map`` is [n, 4, Hc, Wc]: the env's ``build_obs()["critic_map"]`` in its top-left
        ``[:H, :W]`` corner (cell coordinates stay the ones the vectors carry); elsewhere channel 0
        (obstacles) is 1.0 and channels 1-3 are 0.0 -- an off-map cell cannot be entered, the windows'
        rule (``build_obs_ego``).  With ``canvas == (H, W)`` it is ``build_obs``'s tensor byte for byte.
        ``actor_vec`` [n, A, Dv] and ``critic_vec`` [n, Dg] hold each env's ``build_obs`` rows, normalised
        by its own map's H and W.  No cropping: the canvas must cover every map of the range, with
        Hc, Wc <= 255 and Hc * Wc <= 16384.

        ``rows``: None (every env of the range), or uint8 [E] on the engine's device indexed by env id
        whatever the range (``step_episode``'s ``filled``); the rows of unmarked envs are not written in
        any of the three tensors.  ``which``, ``out`` and ``dtype`` as ``build_obs``.  One launch for the
        canvas and one per same-shape run of the range for the vectors, none of them synchronising with
        the host: the call can be captured in a hipGraph."""
        dt = _obs_dtype(dtype)
        Hc, Wc = self._canvas(canvas)
        env_begin = int(env_begin)
        n = self.E - env_begin if n is None else int(n)
        if env_begin < 0 or n < 0 or env_begin + n > self.E:
            raise IndexError(f"env range [{env_begin}, {env_begin + n}) outside [0, {self.E})")
        if rows is not None:
            self._check_mask(rows, "rows")
        if out is None:
            out = self.canvas_buffers((Hc, Wc), n, dtype)
            if rows is not None:   # unmarked rows of a fresh tensor read as zeros
                for t in out.values():
                    t.zero_()
        shapes = dict(actor_vec=(n, self.A, self.actor_vec_dim), critic_map=(n, 4, Hc, Wc),
                      critic_vec=(n, self.critic_vec_dim))
        op = []
        for k in self.CANVAS_KEYS:
            t = out[k] if k in which else None
            if t is not None:
                self._check_obs_out(t, k, shapes[k], dtype)
            op.append(ptr(t))
        if n == 0:
            return out
        check(lib().mdl_build_obs_canvas(self._h, env_begin, n, ptr(rows), dt, Hc, Wc, *op, self._stream()),
              "mdl_build_obs_canvas")
        return out

    # ---- IDQ / qmix featurizers ----
    def build_obs_alt(self, env_begin: int = 0, n: int | None = None, out: dict | None = None,
                      state_shape=None, which=("idq_obs", "qmix_state")):
        """convert_state for every agent (IDQ/networks.py:112-217, == qmix/networks.py:243-348) and
        convert_global_state_to_tensor (qmix/networks.py:350-468) for envs [env_begin, env_begin+n).
        state_shape (7, h, w) defaults to the map's (7, H, W) as the qmix trainer uses; build the
        engine with tracker="fresh" for the IDQ / qmix trainers' per-episode trackers."""
        n, g = self._obs_range(env_begin, n)
        out, op = self._alt_out(out, n, *g.shape, state_shape, new=which)
        if n == 0:
            return out
        check(lib().mdl_build_obs_alt(self._h, env_begin, n, *op, self._stream()), "mdl_build_obs_alt")
        return out

    def build_obs_alt_ego(self, radius: int, env_begin: int = 0, n: int | None = None,
                          rows: torch.Tensor | None = None, out: torch.Tensor | None = None):
        """Each robot's ``K x K`` window of its ``idq_obs`` (``build_obs_alt``: convert_state), centred on
        the robot (K = 2 * radius + 1, radius in 1..15), for envs [env_begin, env_begin + n): a float32
        tensor [n, A, 6, K, K].

        ``ego[e, a, ch, i, j] = build_obs_alt()["idq_obs"][e, a, ch, r - radius + i, c - radius + j]`` for
        robot a on cell (r, c) where that cell lies inside the map -- same tracker mode and clock, channel
        1 the same float32 urgency bits.  Outside the map channel 0 is 1.0 and channels 1-5 are 0.0, so
        channel 4 is a single 1.0 at (radius, radius).  A carrying robot's channels 1 and 2 are zero, and
        its carried target (channel 5) may fall outside the window.  The shape does not depend on the
        map, so the range may cross map shapes (``build_obs_alt`` refuses that).

        float32 only: the urgency plane would not survive a half type exactly and the replay rings hold
        float rows; these windows have no half form.

        ``rows``: None, or uint8 [E] on the engine's device, indexed by env id whatever the range; a
        non-zero byte = build.  The launch reads the mask itself (no host round trip, so the call can be
        captured in a hipGraph).  The rows of unmarked envs are not written -- in a caller's ``out`` they
        keep what they held, and a fresh tensor (``out=None``) starts as zeros.  ``out``: a contiguous
        float32 tensor on the engine's device with n * A * 6 * K * K entries."""
        R = self._ego_radius(radius)
        K = 2 * R + 1
        if rows is not None:
            self._check_mask(rows, "rows")
        env_begin = int(env_begin)
        n = self.E - env_begin if n is None else int(n)
        if env_begin < 0 or n < 0 or env_begin + n > self.E:
            raise IndexError(f"env range [{env_begin}, {env_begin + n}) outside [0, {self.E})")
        need = n * self.A * 6 * K * K
        if out is None:
            make = torch.empty if rows is None else torch.zeros
            out = make((n, self.A, 6, K, K), dtype=torch.float32, device=self.device)
        else:
            self._check_buf(out, torch.float32, need, (TypeError, "out must be a float32 tensor"),
                            (ValueError, f"out must be contiguous on {self.device}"),
                            (ValueError, f"out holds {{n}} entries, needs {need} ({n}, {self.A}, 6, {K}, {K})"))
        if n == 0:
            return out
        check(lib().mdl_build_obs_alt_ego(self._h, env_begin, n, ptr(rows), R, ptr(out), self._stream()),
              "mdl_build_obs_alt_ego")
        return out

    def alt_pre_buffer(self) -> torch.Tensor:
        """The pre-record of ``alt_transition`` (uint8, ``mdl_alt_pre_bytes`` long): what
        reward_shaping reads of the state and the tracker from before a step."""
        nb = C.c_int64(0)
        check(lib().mdl_alt_pre_bytes(self._h, C.byref(nb)), "mdl_alt_pre_bytes")
        return torch.zeros(nb.value, dtype=torch.uint8, device=self.device)

    def alt_transition(self, actions, pre: torch.Tensor, row_mask: torch.Tensor | None = None,
                       ops_are_ints: bool = False, out: dict | None = None, state_shape=None, which=("idq_obs",),
                       action_format: str = "int", r_out: torch.Tensor | None = None):
        """The IDQ trainer's work after a step (IDQ/trainer.py:286-311) for all E envs: per-agent
        reward_shaping (IDQ/networks.py:228-349) of the transition the engine just made with
        ``actions`` (uint8 [E, A]), from ``pre`` (``alt_pre_buffer()``: the record the previous
        call left of the state and tracker before the step), then the new record and
        ``build_obs_alt``'s observations of the new state.  An env whose byte of ``row_mask``
        (uint8 [E], e.g. ``step_episode``'s ``filled``) is 0 gets reward 0 and keeps its rows of
        the observations and of ``pre``.  ``actions=None`` is the begin form (after a reset): no
        reward.  ops_are_ints=False reproduces the trainer, which hands reward_shaping string
        ops.  Returns (r_idq f64 [E, A] or None, obs dict)."""
        n = self.E
        H, W = self.single_map_shape("alt_transition")
        nb = n * self.A * 16 + n * 4
        self._check_buf(pre, torch.uint8, nb,
                        (TypeError, f"pre must be a contiguous uint8 tensor on {self.device} (alt_pre_buffer())"),
                        short=(ValueError, f"pre holds {{n}} bytes, needs {nb}"))
        if row_mask is not None:
            self._check_mask(row_mask, "row_mask")
        out, op = self._alt_out(out, n, H, W, state_shape, new=which, which=which)
        if actions is not None:
            actions = self._step_args(actions, n)
            if r_out is None:
                r_out = torch.empty((n, self.A), dtype=torch.float64, device=self.device)
            else:
                self._check_buf(r_out, torch.float64, n * self.A, (
                    TypeError, f"r_out must be a contiguous float64 tensor of {n * self.A} entries on {self.device}"))
        else:
            r_out = None
        check(lib().mdl_alt_transition(self._h, ptr(actions), ACTION_FORMATS[action_format], 1 if ops_are_ints else 0,
                                       ptr(row_mask), pre.data_ptr(), ptr(r_out), *op, self._stream()),
              "mdl_alt_transition")
        self._keep = (None, actions)
        return r_out, {k: out[k] for k in ALT_KEYS if k in which and out.get(k) is not None}

    def cycle_begin(self, done: torch.Tensor, out: dict | None = None, completed: torch.Tensor | None = None,
                    completed_return: torch.Tensor | None = None, completed_steps: torch.Tensor | None = None,
                    state_shape=None):
        """The lazy reset that opens a time step of the map-QMIX cycle (qmix/trainer.py:329-346), one
        launch over all E envs.  An env whose byte of ``done`` (uint8 [E], read and cleared on the
        device) is set reports its finished episode -- completed[e] = 1, completed_return[e] = its
        total_reward, completed_steps[e] = its t --, has its tracker emptied and is reset (exactly
        ``clear_tracker(ids)`` then ``reset(ids)``), and rows e of ``out["idq_obs"]`` /
        ``out["qmix_state"]`` receive ``build_obs_alt``'s observations of the new state.  Any other
        env gets completed 0, return 0.0, steps 0 and keeps its state and its rows.  ``out`` holds the
        caller's tensors (either may be missing); completed uint8, completed_return float64,
        completed_steps int32, each [E] or None.  Returns ``out``."""
        n = self.E
        H, W = self.single_map_shape("cycle_begin")
        self._check_mask(done, "done")
        out, op = self._alt_out(out, n, H, W, state_shape)
        if completed is not None:
            self._check_mask(completed, "completed")
            if completed.data_ptr() == done.data_ptr():
                raise ValueError("completed must not be the done mask itself (the launch reads one and writes both)")
        for t, dt, name in ((completed_return, torch.float64, "completed_return"),
                            (completed_steps, torch.int32, "completed_steps")):
            if t is not None:
                self._check_buf(t, dt, n, (TypeError, f"{name} must be a contiguous {dt} tensor of {n} entries on "
                                                      f"{self.device}"))
        check(lib().mdl_cycle_begin(self._h, done.data_ptr(), ptr(completed), ptr(completed_return),
                                    ptr(completed_steps), *op, self._stream()), "mdl_cycle_begin")
        return out

    # ---- greedy baseline: greedyagent.py batched on the device ----
    def greedy_init(self, env_ids=None):
        """``GreedyAgents()`` + ``init_agents(state)`` for the listed envs (right after their reset)."""
        ids, n = self._ids(env_ids)
        if n == 0 and env_ids is not None:
            return
        check(lib().mdl_greedy_init(self._h, ptr(ids), n, self._stream()), "mdl_greedy_init")
        self._keep_g = ids

    def greedy_actions(self, env_ids=None, out=None) -> torch.Tensor:
        """One ``get_actions(state)`` per listed env: uint8 [n, A] in the "codes" action format."""
        ids, n = self._ids(env_ids)
        if out is None:
            out = torch.empty((n, self.A), dtype=torch.uint8, device=self.device)
        else:
            self._check_buf(out, torch.uint8, n * self.A, (
                ValueError, f"out must be a contiguous uint8 tensor on {self.device} of >= {n}x{self.A} entries"))
        if n == 0:
            return out
        check(lib().mdl_greedy_actions(self._h, ptr(ids), n, ptr(out), self._stream()), "mdl_greedy_actions")
        self._keep_g = ids
        return out

    def greedy_actions_masked(self, active, out=None) -> torch.Tensor:
        """``greedy_actions()`` for an episode batch: uint8 [E, A] in the "codes" format, row e = env e.
        An env whose byte of ``active`` (uint8 [E] on the device, ``step_episode``'s mask; read, never
        written) is 0 gets the all-zero row ('S', '0') and is not touched -- its agent record stays as
        it is.  ``active=None``: every env, exactly ``greedy_actions()``.  One launch, no host round trip."""
        if active is not None:
            self._check_mask(active, "active")
        if out is None:
            out = torch.empty((self.E, self.A), dtype=torch.uint8, device=self.device)
        else:
            self._check_buf(out, torch.uint8, self.E * self.A, (
                ValueError, f"out must be a contiguous uint8 tensor on {self.device} of >= {self.E}x{self.A} entries"))
        check(lib().mdl_greedy_actions_masked(self._h, ptr(active), ptr(out), self._stream()),
              "mdl_greedy_actions_masked")
        return out

    def episode_results(self, out=None):
        """(total_reward f64 [E], delivered int32 [E], steps int32 [E]) of every env: its fp64
        ``total_reward``, the number of its packages whose status is delivered and its ``t`` -- what
        evaluation.py:49-51 reads of a finished episode -- in one small launch, without ``read_state``'s
        tables.  ``out``: three such tensors of >= E entries on the engine's device; an entry may be
        None (that output is not written and None is returned in its place)."""
        if out is None:
            out = (torch.empty(self.E, dtype=torch.float64, device=self.device),
                   torch.empty(self.E, dtype=torch.int32, device=self.device),
                   torch.empty(self.E, dtype=torch.int32, device=self.device))
        else:
            if len(out) != 3:
                raise ValueError("out must be (total_reward, delivered, steps)")
            for t, dt, name in zip(out, (torch.float64, torch.int32, torch.int32), ("total_reward", "delivered", "steps")):
                if t is not None:      # None: an output the caller does not want
                    self._check_vec(t, dt, f"out {name}")
        check(lib().mdl_episode_results(self._h, ptr(out[0]), ptr(out[1]), ptr(out[2]), self._stream()),
              "mdl_episode_results")
        return out[0], out[1], out[2]

    def avail_actions(self, active=None, out=None) -> torch.Tensor:
        """The valid-action mask of every robot in the state the next step acts on: uint8
        [E, A, 15], 1 = available, columns in the trainer-int order (move 'DLRSU'[a % 5], op a // 5).
        A move into a wall or off the map, a pick-up with nothing waiting on the robot's cell or the
        proposed one (or with a package already carried), and a drop whose target is neither cell
        (or with nothing carried) are 0: each is certain to equal a simpler action, whatever the
        other robots do (include/mdl_engine.h, ``mdl_avail_actions``, states the rule).  ('S', 0)
        is always 1.  ``active`` (uint8 [E] on the device, ``step_episode``'s mask; read, never
        written): an env whose byte is 0 gets all ones; None: every env is computed.  ``out``: a
        contiguous uint8 tensor [E, A, 15] on the engine's device.  One launch, no host round trip;
        touches no state."""
        if active is not None:
            self._check_mask(active, "active")
        shape = (self.E, self.A, ACTION_DIM)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        else:
            self._check_buf(out, torch.uint8, shape, (
                ValueError, f"out must be a contiguous uint8 tensor {list(shape)} on {self.device}"))
        check(lib().mdl_avail_actions(self._h, ptr(active), ptr(out), self._stream()), "mdl_avail_actions")
        return out

    # ---- checkpoint: engine state incl. every env's MT19937 stream ----
    def save_state(self, path=None) -> np.ndarray:
        """Snapshot of the whole engine state as a uint8 array (written to ``path`` as .npy
        when given).  Loading it into an engine built with the same configuration resumes
        every env exactly (the reference cannot: its RandomState lives inside each env)."""
        n = C.c_int64()
        check(lib().mdl_state_bytes(self._h, C.byref(n)), "mdl_state_bytes")
        buf = np.zeros(n.value, np.uint8)
        check(lib().mdl_save_state(self._h, buf.ctypes.data, n.value, self._stream()), "mdl_save_state")
        if path is not None:
            np.save(path, buf, allow_pickle=False)
        return buf

    def load_state(self, src) -> None:
        """Restore a ``save_state`` snapshot (array or .npy path); raises on a mismatched engine."""
        buf = np.load(src, allow_pickle=False) if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__") \
            else np.asarray(src)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        check(lib().mdl_load_state(self._h, buf.ctypes.data, buf.nbytes, self._stream()), "mdl_load_state")

    # ---- dict-API mailbox (include/mdl_engine.h: mdl_mailbox / mdl_mail_*) ----
    def mailbox(self) -> dict:
        """numpy views of the engine's host-mapped mailbox (allocated on first use): inputs
        ``codes`` [E, A] (MDL_ACTION_CODES bytes) and ``ids`` [E]; outputs, row w = the w-th env
        of the last call: ``r_env``, ``r_shaped``, ``done``, ``robots`` [E, A, 3], ``pkgs``
        [E, P, 8], ``t``, ``total_reward``, ``rterms`` (the MDL_RTERM_* bits of the reward
        terms the step added).  The device reads the inputs and writes the outputs in place;
        every ``mail_*`` call returns once its rows are there (it spins on a completion word)."""
        mb = self.__dict__.get("_mb")
        if mb is None:
            m = _lib.MdlMailbox()
            check(lib().mdl_mailbox(self._h, C.byref(m)), "mdl_mailbox")
            E, A, P = self.E, self.A, self.P

            def arr(addr, ctype, shape):
                n = 1
                for d in shape:
                    n *= d
                return np.ctypeslib.as_array((ctype * n).from_address(addr)).reshape(shape)
            mb = dict(codes=arr(m.codes, C.c_uint8, (E, A)), ids=arr(m.ids, C.c_int32, (E,)),
                      r_env=arr(m.r_env, C.c_double, (E,)), r_shaped=arr(m.r_shaped, C.c_float, (E,)),
                      done=arr(m.done, C.c_uint8, (E,)), robots=arr(m.robots, C.c_int32, (E, A, 3)),
                      pkgs=arr(m.pkgs, C.c_int32, (E, P, 8)), t=arr(m.t, C.c_int32, (E,)),
                      total_reward=arr(m.total_reward, C.c_double, (E,)), rterms=arr(m.rterms, C.c_int32, (E,)))
            self._mb = mb
            self._mbox = m
            L = lib()
            self._mail_fns = (L.mdl_mail_step, L.mdl_mail_reset, L.mdl_mail_export)
        return mb

    def mail_ctx(self):
        """The mailbox as the C extension's context (compat.Environment.step in one C call)."""
        c = self.__dict__.get("_mail_ctx")
        if c is None:
            self.mailbox()
            m = self._mbox
            c = self._mail_ctx = _lib.pack().mail_ctx(
                C.cast(lib().mdl_mail_step, C.c_void_p).value, self._h.value, m.codes, m.ids, m.r_env, m.done,
                m.robots, m.pkgs, m.t, m.total_reward, m.rterms, self.A, self.P)
        return c

    def mail_step(self, n: int, use_ids: bool, auto_reset: bool = False) -> None:
        """Step the mailbox's envs (``ids[:n]`` when use_ids, else all E, with ``codes[:n]``) and
        bring their rows into the mailbox: one step launch + one export launch, then a spin."""
        rc = self._mail_fns[0](self._h, n, 1 if use_ids else 0, 1 if auto_reset else 0, _raw_stream(self._dev))
        if rc:
            check(rc, "mdl_mail_step")

    def mail_reset(self, n: int, use_ids: bool) -> None:
        rc = self._mail_fns[1](self._h, n, 1 if use_ids else 0, _raw_stream(self._dev))
        if rc:
            check(rc, "mdl_mail_reset")

    def mail_export(self, n: int, use_ids: bool) -> None:
        rc = self._mail_fns[2](self._h, n, 1 if use_ids else 0, _raw_stream(self._dev))
        if rc:
            check(rc, "mdl_mail_export")

    def read_state(self):
        """int32/f64 device tensors: robots [E,A,3] (r,c,carry), pkgs [E,P,8]
        (sr,sc,tr,tc,start_time,deadline,id,status), t [E], total_reward [E],
        tracker [E,P,4] (present,in_transit,order,_), tracker_data [E,P,6]."""
        i = dict(dtype=torch.int32, device=self.device)
        s = dict(robots=torch.empty((self.E, self.A, 3), **i), pkgs=torch.empty((self.E, self.P, 8), **i),
                 t=torch.empty(self.E, **i), total_reward=torch.empty(self.E, dtype=torch.float64, device=self.device),
                 tracker=torch.empty((self.E, self.P, 4), **i), tracker_data=torch.empty((self.E, self.P, 6), **i))
        check(lib().mdl_read_state(self._h, ptr(s["robots"]), ptr(s["pkgs"]), ptr(s["t"]), ptr(s["total_reward"]),
                                   ptr(s["tracker"]), ptr(s["tracker_data"]), self._stream()), "mdl_read_state")
        return s

    def tracker_rows(self, state_cpu: dict, e: int) -> np.ndarray:
        """Tracker of env e as ordered dict rows (id, status, sr, sc, tr, tc, st, dl)."""
        trk = state_cpu["tracker"][e]
        data = state_cpu["tracker_data"][e]
        pres = np.nonzero(trk[:, 0])[0]
        order = pres[np.argsort(trk[pres, 2], kind="stable")]
        rows = np.zeros((len(order), 8), np.int32)
        rows[:, 0] = order + 1
        rows[:, 1] = np.where(trk[order, 1] != 0, 2, 1)
        rows[:, 2:8] = data[order]
        return rows
