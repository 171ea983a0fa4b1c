"""The reference for half-precision observations (BatchedEnv.build_obs(dtype=), step_obs(obs_dtype=),
MappoRollout(obs_dtype=)): every element is the float32 observation rounded once to nearest-even, i.e.
torch's CPU conversion of the float32 tensor, compared as bit patterns.  Also the predicates the
rounding-edge tests use to show that an input really holds the edge they mean to check.

This module only holds helpers; it is not a conftest."""
from __future__ import annotations

import numpy as np
import torch

HALF_DTYPES = (torch.float16, torch.bfloat16)
OBS_KEYS = ("actor_map", "actor_vec", "critic_map", "critic_vec")


def round_to(x, dtype):
    """float32 array -> the uint16 bit patterns of ``x`` converted to ``dtype`` on the CPU (RNE)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    t = torch.from_numpy(x).to(dtype)
    return t.view(torch.int16).numpy().view(np.uint16)


def bits16(t):
    """A half tensor (any device) -> its uint16 bit patterns."""
    assert t.dtype in HALF_DTYPES, t.dtype
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def has_tie(x, dtype):
    """Whether some element of the float32 array lies exactly half way between two neighbours of
    ``dtype``: bf16 keeps 16 of the 32 bits (low 16 == 0x8000); fp16 keeps 10 mantissa bits of 23
    (low 13 == 0x1000) where the value is in fp16's normal range (2^-14 <= |x| < 2^16)."""
    u = _u32(x)
    e = (u >> 23) & 0xFF
    if dtype == torch.bfloat16:
        return bool((((u & 0xFFFF) == 0x8000) & (e != 0xFF)).any())
    assert dtype == torch.float16
    return bool((((u & 0x1FFF) == 0x1000) & (e >= 127 - 14) & (e <= 127 + 15)).any())


def has_fp16_subnormal(x):
    """Whether some element is non-zero, below fp16's smallest normal (2^-14), not representable
    exactly and still rounds to a non-zero fp16 subnormal (a flush to zero would change it)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.abs(x)
    sub = (a > 0) & (a < np.float32(2.0 ** -14))
    h = x.astype(np.float16)
    return bool((sub & (h != 0) & (h.astype(np.float32) != x)).any())
