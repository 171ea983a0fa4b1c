"""Action selection on the device: the policy sampler and the epsilon-greedy selection, each with a
``_dev`` form whose offset base (and epsilon) is read on the device so the launch can live in a
replayed hipGraph.  Every draw is the library's own Philox4x32-10 stream keyed by (seed, offset,
row) -- include/mdl_engine.h states it exactly --: deterministic, independent of launch shape."""
from __future__ import annotations

import torch

from ._lib import check, lib, ptr, stream_handle

ACTION_DIM = 15  # MAPPO/trainer.py:41; QMIX/trainer.py: num_move_actions * num_pkg_ops
_U64 = 2**64 - 1


def _avail_rows(avail, shape, what):
    """``avail`` as the kernels read it: contiguous uint8 of ``shape`` ([rows, n_actions])."""
    if avail.numel() != shape[0] * shape[1] or avail.shape[-1] != shape[1]:
        raise ValueError(f"avail must have {what}'s shape")
    if avail.dtype != torch.uint8 or not avail.is_contiguous():
        avail = avail.to(torch.uint8).contiguous()
    return avail


def _sample(name, logits, seed, offset_dev, offset, out, avail=None):
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        logits = logits.float().contiguous()
    N, n_act = logits.shape
    if out is None:
        out = (torch.empty(N, dtype=torch.uint8, device=logits.device),
               torch.empty(N, dtype=torch.float32, device=logits.device))
    acts, lp = out
    base = () if offset_dev is None else (ptr(offset_dev),)
    mask = ()
    if avail is not None:   # the masked entry point: mdl_sample_actions[_dev] -> mdl_sample_actions_avail[_dev]
        name = name.replace("mdl_sample_actions", "mdl_sample_actions_avail")
        mask = (ptr(_avail_rows(avail, (N, n_act), "logits")),)
    check(getattr(lib(), name)(ptr(logits), *mask, N, n_act, seed & _U64, *base, offset & _U64, ptr(acts), ptr(lp),
                               stream_handle(logits.device)), name)
    return acts, lp


def sample_actions(logits: torch.Tensor, seed: int, offset: int, out=None, avail=None):
    """``Categorical(logits=logits).sample()`` and ``.log_prob`` (MAPPO/trainer.py:141-143).

    logits: float32 [N, n_actions] on the device.  Returns (actions uint8 [N],
    log_probs float32 [N]).  The draw is the library's own Philox4x32-10 stream
    keyed by (seed, offset, row): deterministic, independent of launch shape.
    avail: bool/uint8 with N rows of n_actions (``BatchedEnv.avail_actions``'s [E, A, 15]
    for [E*A, 15] logits) or None (= every action available): the draw and the log-prob
    are those of the softmax over the available actions only; an unavailable action is
    never returned.  An all-ones avail gives None's results bit for bit.
    """
    return _sample("mdl_sample_actions", logits, seed, None, offset, out, avail)


def sample_actions_dev(logits: torch.Tensor, seed: int, offset_dev: torch.Tensor, offset_add: int, out, avail=None):
    """``sample_actions`` at offset ``offset_dev[0] + offset_add`` with the base read on the
    device (uint64 tensor [1]), so the launch can live in a replayed hipGraph."""
    return _sample("mdl_sample_actions_dev", logits, seed, offset_dev, offset_add, out, avail)


def _select(name, q, epsilon, seed, offset_dev, offset, avail, out, mark=False, explored=None):
    """One epsilon-greedy launch.  offset_dev None: epsilon is a float and offset the whole offset;
    otherwise epsilon is the device tensor and the offset is ``offset_dev[0] + offset``.
    mark: also report the rows that explored (into ``explored`` if given)."""
    if q.dtype != torch.float32 or not q.is_contiguous():
        q = q.float().contiguous()
    if q.dim() != 2:
        raise ValueError("q must be [rows, n_actions]")
    N, n_act = q.shape
    if avail is not None:
        avail = _avail_rows(avail, (N, n_act), "q")
    if offset_dev is None:
        eps, base = float(epsilon), ()
    else:
        if epsilon.dtype != torch.float32 or offset_dev.dtype != torch.int64:
            raise TypeError("epsilon_dev must be float32 and offset_dev int64 (uint64 bits)")
        eps, base = ptr(epsilon), (ptr(offset_dev),)
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=q.device)
    if mark and explored is None:
        explored = torch.empty(N, dtype=torch.uint8, device=q.device)
    marks = (ptr(explored),) if mark else ()
    check(getattr(lib(), name)(ptr(q), ptr(avail), N, n_act, eps, seed & _U64, *base, offset & _U64, ptr(out), *marks,
                               stream_handle(q.device)), name)
    return (out, explored) if mark else out


def select_actions_eps(q: torch.Tensor, epsilon: float, seed: int, offset: int, avail=None, out=None):
    """Epsilon-greedy selection over Q-values (QMIX/trainer.py:298-319).

    q: float32 [N, n_actions] on the device; avail: bool/uint8 of the same shape (or with the
    rows split, ``BatchedEnv.avail_actions``'s [E, A, n_actions]) or None (= every action
    available).  Returns actions uint8 [N].  A row explores with
    probability epsilon and then takes a uniformly drawn available action; otherwise it
    takes the first available action with the largest q.  The draw is the library's own
    Philox4x32-10 stream keyed by (seed, offset, row) -- include/mdl_engine.h states it
    exactly --: deterministic, independent of launch shape."""
    return _select("mdl_select_actions_eps", q, epsilon, seed, None, offset, avail, out)


def select_actions_eps_dev(q: torch.Tensor, epsilon_dev: torch.Tensor, seed: int, offset_dev: torch.Tensor,
                           offset_add: int, avail=None, out=None):
    """``select_actions_eps`` with epsilon (float32 tensor [1]) and the offset base (uint64
    bits in an int64 tensor [1]; the offset is ``offset_dev[0] + offset_add``) read on the
    device, so the launch can live in a replayed hipGraph."""
    return _select("mdl_select_actions_eps_dev", q, epsilon_dev, seed, offset_dev, offset_add, avail, out)


def select_actions_eps_mark(q: torch.Tensor, epsilon: float, seed: int, offset: int, avail=None, out=None,
                            explored=None):
    """``select_actions_eps`` (the same actions, bit for bit) that also reports which rows explored:
    returns (actions uint8 [N], explored uint8 [N]); explored is 1 where the row's uniform fell
    below epsilon and the row had an available action."""
    return _select("mdl_select_actions_eps_mark", q, epsilon, seed, None, offset, avail, out,
                   True, explored)


def select_actions_eps_mark_dev(q: torch.Tensor, epsilon_dev: torch.Tensor, seed: int, offset_dev: torch.Tensor,
                                offset_add: int, avail=None, out=None, explored=None):
    """``select_actions_eps_mark`` with epsilon (float32 tensor [1]) and the offset base (uint64 bits
    in an int64 tensor [1]) read on the device, so the launch can live in a replayed hipGraph."""
    return _select("mdl_select_actions_eps_mark_dev", q, epsilon_dev, seed, offset_dev, offset_add, avail, out,
                   True, explored)
