"""Host model of the device sampler's random numbers (smoltts_amd/csrc/argmax_dev.h), so that tests can predict draws.

``uniform01(seed, slot, frame, step, cols)`` is the counter-based uniform of the device, bit for bit (uint32 arithmetic).  In
slot mode a sampled row uses the *request key* ``uniform01(seed, 0, frame, step, col)``: the request's own 64-bit seed, unsalted,
its own frame number (0 at its frame 0), the step (0 = slow token, i = depth code i - 1) and the column.

``gumbel_pick`` models the pick itself: the first index of the largest ``(logit - max) / temp - log(-log(u))`` over the columns
with ``p >= min_p * p_max``.  The device evaluates ``logf`` in fp32, so where the two largest keys lie within a few ulp the
model may name the other one; ``gumbel_keys`` gives the keys to check that margin.
"""
from __future__ import annotations

import numpy as np

_M1, _M2 = np.uint32(0x7FEB352D), np.uint32(0x846CA68B)


def mix32(x):
    x = np.asarray(x, dtype=np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * _M1
        x = x ^ (x >> np.uint32(15))
        x = x * _M2
        x = x ^ (x >> np.uint32(16))
    return x


def _u32(v: int) -> np.uint32:
    return np.uint32(int(v) & 0xFFFFFFFF)


def uniform01(seed: int, slot: int, frame: int, step: int, cols) -> np.ndarray:
    """float32 uniforms in (0, 1) of columns ``cols`` (array of ints)."""
    seed = int(seed) & (2**64 - 1)
    cols = np.asarray(cols, dtype=np.int64)
    with np.errstate(over="ignore"):
        h = mix32(_u32(seed) ^ (np.uint32(0x9E3779B9) * _u32(slot + 1)))
        h = mix32(h ^ _u32(seed >> 32) ^ (np.uint32(0x85EBCA6B) * _u32(frame + 1)))
        h = mix32(h ^ (np.uint32(0xC2B2AE35) * _u32(step + 1)))
        h = mix32(h ^ (np.uint32(0x27D4EB2F) * (cols + 1).astype(np.uint32)))
    return (((h >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def request_uniforms(seed: int, frame: int, step: int, n_cols: int) -> np.ndarray:
    """The request key's uniforms of one row (slot mode)."""
    return uniform01(seed, 0, frame, step, np.arange(n_cols))


def gumbel_keys(logits, temp: float, min_p: float, seed: int, frame: int, step: int) -> np.ndarray:
    """float64 keys of one row under the request key; -inf where min_p removes the column."""
    x = np.asarray(logits, dtype=np.float32)
    z = ((x - x.max()) * np.float32(1.0 / np.float32(temp))).astype(np.float64)
    u = request_uniforms(seed, frame, step, x.shape[0]).astype(np.float64)
    key = z - np.log(-np.log(u))
    if min_p > 0:
        key[z < np.log(np.float32(min_p))] = -np.inf
    return key


def gumbel_pick(logits, temp: float, min_p: float, seed: int, frame: int, step: int) -> int:
    """The column a sampled row picks (temp > 0); temp <= 0: the first maximum (greedy)."""
    x = np.asarray(logits, dtype=np.float32)
    if temp <= 0:
        return int(np.argmax(x))
    return int(np.argmax(gumbel_keys(x, temp, min_p, seed, frame, step)))
