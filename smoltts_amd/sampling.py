"""Host model of the device sampler's random numbers (smoltts_amd/csrc/argmax_dev.h), so that tests can predict draws.

``uniform01(seed, slot, frame, step, cols)`` is the counter-based uniform of the device, bit for bit (uint32 arithmetic).  In
slot mode a sampled row uses the *request key* ``uniform01(seed, 0, frame, step, col)``: the request's own 64-bit seed, unsalted,
its own frame number (0 at its frame 0), the step (0 = slow token, i = depth code i - 1) and the column.

``gumbel_pick`` models the pick itself: the first index of the largest ``(logit - max) / temp - log(-log(u))`` over the columns
with ``p >= min_p * p_max``.  The device evaluates ``logf`` in fp32, so where the two largest keys lie within a few ulp the
model may name the other one; ``gumbel_keys`` gives the keys to check that margin.

``filtered_keys`` / ``filtered_pick`` model the per-request filters of a sampled row (``SmolttsSlotFilters``), in the
device's order: repetition penalty over the history ids, ``top_k``, ``top_p``, then ``min_p`` and the unchanged Gumbel key.  The
device sums fp32 ``expf`` masses (rounded down to multiples of 2^-40, exactly); a row whose nucleus edge lies within
``TOP_P_EDGE_MARGIN`` (relative) of ``top_p`` may keep or drop its edge column there: ``top_p_edge`` names that column.

``length_patch`` models the per-request length control of the slow pick (``SmolttsSlotLength``): the row a pick
sees, in front of everything above.  It is exact: one rounded fp32 add, or a store of -inf.

``pick_logprob`` models the score of the slow pick (``smoltts_session_set_slot_score``): the log-probability, at
temperature 1, of the emitted id under the row the pick saw.  The device's ``expf`` is the only inexact step:
``LOGPROB_MARGIN`` bounds what it can move.
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


MAX_REPETITION_WINDOW = 64
MAX_REPETITION_PENALTY = 10.0  # of the public interface (RequestSampling); the fish-speech family runs 1.0 .. 2.0
# fp32 expf (about 2 ulp: 1.2e-7 relative per column) and the 2^-40 quantum of the device's mass sums stay below 1e-6 of the
# total; x 10
TOP_P_EDGE_MARGIN = 1e-5
# the same two sources bound the relative error of the score's mass sum S below 1e-6, which is the absolute error of log S (a CPU
# simulation with expf biased by +-3 ulp over rows of 5 .. 65,836 columns gave 3e-7); x 10.  Absolute, per pick.
LOGPROB_MARGIN = 1e-5


def penalised_row(logits, penalty: float, history) -> np.ndarray:
    """The fp32 row after the repetition penalty: each distinct in-range id of ``history`` once, ``x * fp32(1 / r)`` if
    ``x > 0`` else ``x * r`` (one rounded fp32 multiply)."""
    x = np.array(logits, dtype=np.float32, copy=True)
    hist = np.unique(np.asarray(history if history is not None else [], dtype=np.int64))
    hist = hist[(hist >= 0) & (hist < x.shape[0])]
    if penalty > 1 and hist.size:
        r = np.float32(penalty)
        inv = np.float32(1.0) / r
        x[hist] = np.where(x[hist] > 0, x[hist] * inv, x[hist] * r).astype(np.float32)
    return x


def _z32(x: np.ndarray, temp: float) -> np.ndarray:
    return ((x - x.max()) * np.float32(1.0 / np.float32(temp))).astype(np.float32)


def _top_k_keep(x: np.ndarray, top_k: int) -> np.ndarray:
    if not 0 < top_k < x.shape[0]:
        return np.ones(x.shape[0], dtype=bool)
    return x >= np.sort(x)[x.shape[0] - top_k]  # the k-th largest, duplicates counted; ties stay


def _mass_above(z: np.ndarray, keep: np.ndarray):
    """(mass of the kept columns with z strictly greater than each column's z, total mass of the kept columns), float64."""
    p = np.where(keep, np.exp(z.astype(np.float64)), 0.0)
    uz, inv = np.unique(z, return_inverse=True)  # ascending
    group = np.bincount(inv, weights=p, minlength=uz.shape[0])
    above = np.concatenate([np.cumsum(group[::-1])[::-1][1:], [0.0]])
    return above[inv], float(p.sum())


def filter_keep(logits, temp: float, top_k: int = 0, top_p: float = 1.0, penalty: float = 1.0, history=None):
    """(penalised fp32 row, z of its columns, bool mask of the columns top_k and top_p keep)."""
    x = penalised_row(logits, penalty, history)
    z = _z32(x, temp)
    keep = _top_k_keep(x, int(top_k))
    if 0 < top_p < 1:
        above, total = _mass_above(z, keep)
        keep = keep & (above < float(np.float32(top_p)) * total)
    return x, z, keep


def filtered_keys(logits, temp: float, min_p: float, seed: int, frame: int, step: int, top_k: int = 0, top_p: float = 1.0,
                  penalty: float = 1.0, history=None) -> np.ndarray:
    """float64 keys of one sampled row under the request key; -inf where the penalty + top_k + top_p + min_p chain removes
    the column.  With the three filters off these are ``gumbel_keys``."""
    x, z, keep = filter_keep(logits, temp, top_k, top_p, penalty, history)
    u = request_uniforms(seed, frame, step, x.shape[0]).astype(np.float64)
    key = z.astype(np.float64) - np.log(-np.log(u))
    key[~keep] = -np.inf
    if min_p > 0:
        key[z.astype(np.float64) < np.log(np.float32(min_p))] = -np.inf
    return key


def filtered_pick(logits, temp: float, min_p: float, seed: int, frame: int, step: int, top_k: int = 0, top_p: float = 1.0,
                  penalty: float = 1.0, history=None) -> int:
    """The column a row picks with its filters; a greedy row (temp <= 0) ignores them: the first maximum of the raw row."""
    if temp <= 0:
        return int(np.argmax(np.asarray(logits, dtype=np.float32)))
    return int(np.argmax(filtered_keys(logits, temp, min_p, seed, frame, step, top_k, top_p, penalty, history)))


def top_p_edge(logits, temp: float, top_k: int = 0, top_p: float = 1.0, penalty: float = 1.0, history=None):
    """(edge column, relative distance): the column (the first of its tie group) whose threshold mass -- the mass of the kept
    columns strictly more probable than it, over the total -- lies closest to ``top_p``, and ``|that - top_p| / top_p``.  Only
    the columns of this group can differ between the model and the device, and only when the distance is below
    ``TOP_P_EDGE_MARGIN``.  ``top_p`` off: (-1, inf)."""
    if not 0 < top_p < 1:
        return -1, float("inf")
    x = penalised_row(logits, penalty, history)
    z = _z32(x, temp)
    keep = _top_k_keep(x, int(top_k))
    above, total = _mass_above(z, keep)
    tp = float(np.float32(top_p))
    dist = np.where(keep, np.abs(above / total - tp) / tp, np.inf)
    j = int(np.argmin(dist))
    return j, float(dist[j])


def length_patch(logits, im_end: int, frame: int, min_frames: int = 0, eos_bias: float = 0.0) -> np.ndarray:
    """The fp32 slow-logit row as the pick of frame ``frame`` sees it under a length entry: ``x[im_end] + fp32(eos_bias)`` (one
    rounded fp32 add), then -inf while ``frame < min_frames``.  An off entry (``min_frames <= 0``, ``eos_bias == 0``) returns
    the row unchanged.  The greedy pick is ``argmax`` of this row; a sampled pick runs its filters and keys on it."""
    x = np.array(logits, dtype=np.float32, copy=True)
    if eos_bias != 0:
        x[im_end] = np.float32(x[im_end]) + np.float32(eos_bias)
    if frame < min_frames:
        x[im_end] = -np.inf
    return x


def pick_logprob(row, picked: int) -> float:
    """The score of one slow pick: ``row`` is the fp32 row as the pick sees it (after ``length_patch`` and ``penalised_row``, before
    temperature, ``top_k``, ``top_p`` and ``min_p``), ``picked`` the id the request emitted.  With ``z = fp32(x - max x)`` (one
    rounded subtract, as on the device), ``q = floor(expf(z) * 2^40)`` and ``S = sum q`` (exact in float64 in any order):
    ``float64(z[picked]) - (log S - 40 ln 2)``, rounded to fp32 as the device stores it.  A column beyond |z| of about 28 has
    mass 0 but a finite score; a -inf column (a length block) contributes nothing."""
    x = np.asarray(row, dtype=np.float32)
    z = _z32(x, 1.0)
    with np.errstate(under="ignore"):
        q = np.floor(np.exp(z, dtype=np.float32).astype(np.float64) * 2.0**40)
    total = float(q.sum())
    return float(np.float32(float(z[int(picked)]) - (np.log(total) - 40.0 * np.log(2.0))))
