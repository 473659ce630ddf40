"""Per-request speaking speed (host side): the speed parser and a numpy model of the GPU time stretch.

Mimi frames are a fixed 12.5 Hz, so a speed other than 1 is a pitch-preserving time-scale modification of the 24 kHz PCM:
WSOLA (waveform-similarity overlap-add) with an integer-exact search.  Output segment k of L samples starts at its nominal
input position ``a_k = (k L speed_q + 2^15) >> 16`` moved by the lag delta in [-DELTA, DELTA] (``p_k = a_k + delta >= 0``)
whose next L samples differ least, as int16 codes summed in int32, from the natural continuation ``p_{k-1} + L`` of the
previous segment; ties go to the smaller |delta|, then to the negative one.  The segments are overlap-added with a periodic
Hann of W = 2L samples.  Every position is an integer function of the int16 codes, so the output does not depend on how the
input is chunked; the GPU kernel (csrc/tsm.hip) and ``Stretcher`` here follow the same steps and differ only by fp32 rounding.

``speed_q == 65536`` is the identity: no state and no launch anywhere.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np

L = 240            # synthesis hop: 10 ms at 24 kHz
W = 2 * L          # window
DELTA = 192        # search tolerance (2 DELTA + 1 = 385 lags)
HIST = 2048        # input samples a stream carries from call to call (at most ~1.9k are ever needed)
SPEED_MIN, SPEED_MAX = 0.25, 4.0
Q_ONE = 65536      # speed 1.0 in Q16


def window() -> np.ndarray:
    """The periodic Hann of W samples, in fp64 and stored as fp32: ``w[n] = 0.5 - 0.5 cos(2 pi n / W)``."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)).astype(np.float32)


def speed_q(speed) -> int:
    """A speed factor (finite, 0.25 <= speed <= 4.0) -> ``round(speed * 65536)``; ``ValueError`` otherwise."""
    try:
        s = float(speed)
    except (TypeError, ValueError):
        raise ValueError(f"speed must be a number, got {speed!r}")
    if not math.isfinite(s) or not SPEED_MIN <= s <= SPEED_MAX:
        raise ValueError(f"speed must be finite and in [{SPEED_MIN}, {SPEED_MAX}], got {speed!r}")
    return int(round(s * Q_ONE))


speed_q_of = speed_q  # (for functions whose own argument is named speed_q)


def parse_speed(speed) -> Optional[int]:
    """``speed_q`` of a request's speed, or None when it asks for none (None, or exactly 1.0 after rounding)."""
    if speed is None:
        return None
    q = speed_q(speed)
    return None if q == Q_ONE else q


def nominal(k: int, sq: int) -> int:
    """a_k, the nominal input position of output segment k."""
    return (k * L * sq + 32768) >> 16


def out_length(n: int, sq: int) -> int:
    """M = ceil(N 65536 / speed_q): the output length of an input of N samples."""
    return -(-(n * Q_ONE) // sq)


def out_bound(n_in: int) -> int:
    """The most output samples one call of ``n_in`` input samples can emit, flush included (smoltts_tsm_out_samples)."""
    return 4 * n_in + 4 * (DELTA + W) + L


def to_s16(x: np.ndarray) -> np.ndarray:
    """The int16 code of every sample, computed in fp32 as the blocking route quantises: ``rint(clip(x, -1, 1) * 32767)``."""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.clip(x, np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)).astype(np.int32)


def _rank(delta: np.ndarray) -> np.ndarray:
    return np.where(delta == 0, 0, np.where(delta < 0, -2 * delta - 1, 2 * delta)).astype(np.int64)


_DELTAS = np.arange(-DELTA, DELTA + 1, dtype=np.int64)
_RANKS = _rank(_DELTAS)


class Stretcher:
    """One stream's WSOLA state: ``push(x, last)`` consumes input samples and returns the output samples that became final.

    The state is that of a GPU slot: the last HIST input samples, the open half-window of L samples, and the counters ``k``
    (next segment), ``p_prev`` (p_{k-1}; -L before segment 0, which makes the first L outputs ``(w[n] + w[n + L]) x[n]``),
    ``n_in`` and ``n_out``.  Segment k is computed once the input holds ``a_k + DELTA + W`` samples and its end ``(k + 1) L``
    does not pass ``out_length(n_in)`` (the second rule binds above speed 2.8 only: nothing past the flush's length is ever
    emitted).  ``last``: the stream ends with this call's samples; the flush treats the input as zero from there on, emits
    segments while ``k L < M`` and cuts the output at exactly M.  ``positions`` lists every chosen p_k."""

    def __init__(self, sq: int):
        if not 16384 <= sq <= 262144:
            raise ValueError(f"speed_q {sq} outside [16384, 262144]")
        self.sq = sq
        self.w = window()
        self.hist = np.zeros(HIST, np.float32)  # input [n_in - HIST, n_in)
        self.ola = np.zeros(L, np.float32)
        self.k, self.p_prev, self.n_in, self.n_out = 0, -L, 0, 0
        self.ended = False
        self.positions: List[int] = []

    def push(self, x, last: bool = False) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        if self.ended:
            return np.zeros(0, np.float32)
        n0 = self.n_in
        buf = np.concatenate([self.hist, x])  # input [n0 - HIST, n0 + len(x))
        base = n0 - HIST
        n1 = n0 + x.size
        mcap = out_length(n1, self.sq)
        out = []
        qbuf = None
        while True:
            a = nominal(self.k, self.sq)
            ok = self.k * L < mcap if last else (a + DELTA + W <= n1 and (self.k + 1) * L <= mcap)
            if not ok:
                break
            hi = a + DELTA + W
            if hi - base > buf.size:  # the flush reads zeros past the end
                buf = np.concatenate([buf, np.zeros(hi - base - buf.size, np.float32)])
                qbuf = None
            if qbuf is None:
                qbuf = to_s16(buf)
            if self.k == 0:
                p = 0
            else:
                ref = qbuf[self.p_prev + L - base: self.p_prev + 2 * L - base]
                lo = a - DELTA - base  # >= 0: a stream never needs input older than HIST samples
                cand = np.lib.stride_tricks.sliding_window_view(qbuf[lo: lo + 2 * DELTA + L], L)
                d = np.abs(cand - ref[None]).sum(axis=1).astype(np.int64)
                keep = a + _DELTAS >= 0
                key = ((d << 32) | _RANKS)[keep]
                p = int(a + _DELTAS[keep][int(np.argmin(key))])
            seg = buf[p - base: p + W - base]
            out.append(self.ola + self.w[:L] * seg[:L])
            self.ola = self.w[L:] * seg[L:]
            self.positions.append(p)
            self.p_prev = p
            self.k += 1
        y = np.concatenate(out) if out else np.zeros(0, np.float32)
        if last:
            y = y[: max(mcap - self.n_out, 0)]
            self.ended = True
        self.n_out += y.size
        self.n_in = n1
        self.hist = np.concatenate([self.hist, x])[-HIST:]
        return y.astype(np.float32)


def stretch(x, speed=None, *, speed_q: Optional[int] = None, return_positions: bool = False):
    """The whole-signal model: ``x`` (float32 at 24 kHz) at the factor ``speed`` (0.25 to 4.0), or at ``speed_q`` (Q16, one of
    the two) -> exactly ``out_length(len(x), speed_q)`` samples; the identity at speed 1.  With ``return_positions``:
    (y, [p_k])."""
    if (speed is None) == (speed_q is None):
        raise ValueError("pass speed or speed_q")
    sq = speed_q_of(speed) if speed is not None else int(speed_q)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if sq == Q_ONE:
        return (x.copy(), []) if return_positions else x.copy()
    st = Stretcher(sq)
    y = st.push(x, last=True)
    return (y, st.positions) if return_positions else y


def stream_chunks(x, sq: int, sizes) -> Tuple[np.ndarray, List[np.ndarray]]:
    """Feed ``x`` in calls of the given sizes (the last call flushes) -> (the concatenated output, the per-call outputs)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    st = Stretcher(sq)
    outs, i = [], 0
    for j, n in enumerate(sizes):
        outs.append(st.push(x[i:i + n], last=j == len(sizes) - 1))
        i += n
    return np.concatenate(outs) if outs else np.zeros(0, np.float32), outs
