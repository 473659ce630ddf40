"""A look-ahead peak limiter for 24 kHz mono speech: the numpy model that defines what ``csrc/limiter.hip`` computes (DESIGN.md
section 22).  The device reproduces it bit for bit: every fp64 operation below is a single rounded multiply, add or divide, a
minimum, a maximum or a compare, in a fixed order; the interpolator is designed here and uploaded, and nothing depends on how
calls cut the stream.

Constants: ``L`` = 120 samples of look-ahead (5 ms), ``R`` = 1200 samples of hold (50 ms), ``HOLD_BACK`` = L + 6 = 126.

Interpolator: for q = 1, 2, 3 and k = -5..6, t = k - q/4 and ``h_q[k] = sinc(t) * (0.5 + 0.5 cos(pi t / 6))``, each phase divided
by its own sum: a Hann-windowed sinc at 4x, 36 doubles.

Peak estimate (samples outside the stream are 0): ``y_q[n] = sum_{k=-5..6} h_q[k] * x[n+k]`` in ascending k,
``p[n] = max(|x[n]|, |y_1[n]|, |y_2[n]|, |y_3[n]|)``.

Required gain: ``r[n] = c / p[n]`` where ``p[n] > c``, else exactly 1.0; ``c = 10^(peak_limit_db / 20)``.  r is 1 outside the stream.

Hold and look-ahead: ``m[n] = min r[n-R .. n+L]``.  m is 1 before the stream.

Smoothing: ``g[n] = min(r[n], (m[n-L] + m[n-L+1] + ... + m[n]) / 121.0)``, summed oldest first.

Output: ``y[n] = float32(double(x[n]) * g[n])``.

``y[n]`` is a function of ``x[n-1325 .. n+126]`` alone, so a stream holds back ``HOLD_BACK`` samples: after ``fed`` samples
``max(0, fed - 126)`` have left, and the rest leaves when the stream ends (zeros assumed behind it).  Where nothing within the
window passes ``c``, 121 ones sum to 121.0, g is exactly 1.0 and the samples leave unchanged bit for bit.

``peak_limit_db`` ranges over [-12, 0] dBFS.  This is a peak limiter on its own 4x estimate, not a certified BS.1770 true-peak
meter.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np

FS = 24000
L = 120                    # look-ahead (5 ms)
R = 1200                   # hold (50 ms)
K_LO, K_HI = -5, 6         # the interpolator's taps
TAPS = K_HI - K_LO + 1
HOLD_BACK = L + K_HI       # samples a stream holds back
WINDOW = R + L + 1         # r values under one m
MEAN = L + 1               # m values under one g
R_HIST = R + 2 * L         # r values a stream keeps: those the held-back samples' gains still read
REACH_BACK = R + L + -K_LO  # y[n] reads x from n - 1325 ...
PEAK_MIN_DB, PEAK_MAX_DB = -12.0, 0.0
MAX_CALL = 61440           # samples one device call takes


def check_peak_limit(db, what: str = "peak_limit_db"):
    """``db`` as a float, or None; ``ValueError`` for anything but a number in [-12, 0]."""
    if db is None:
        return None
    if isinstance(db, bool):
        raise ValueError(f"{what} must be a number of dBFS or null, not a boolean")
    if not isinstance(db, (int, float, np.integer, np.floating)) or not np.isfinite(db):
        raise ValueError(f"{what} must be a number of dBFS between {PEAK_MIN_DB:g} and {PEAK_MAX_DB:g}, or null")
    if not PEAK_MIN_DB <= db <= PEAK_MAX_DB:
        raise ValueError(f"{what} {db:g} outside [{PEAK_MIN_DB:g}, {PEAK_MAX_DB:g}] dBFS")
    return float(db)


def ceiling_of_db(peak_limit_db: float) -> float:
    """c = 10^(peak_limit_db / 20)."""
    return float(10.0 ** (float(peak_limit_db) / 20.0))


def reduction_db(min_gain: float) -> float:
    """-20 log10(min g); 0.0 when the limiter never engaged."""
    g = float(min_gain)
    return 0.0 if g >= 1.0 else float(-20.0 * np.log10(g))


@lru_cache(maxsize=1)
def interpolator() -> np.ndarray:
    """``h``: float64 [3, TAPS], phase q = 1, 2, 3 in row q - 1, tap k at column k + 5 (read-only)."""
    k = np.arange(K_LO, K_HI + 1, dtype=np.float64)
    h = np.zeros((3, TAPS))
    for q in (1, 2, 3):
        t = k - q / 4.0
        w = np.sinc(t) * (0.5 + 0.5 * np.cos(np.pi * t / 6.0))
        h[q - 1] = w / np.sum(w)
    h.setflags(write=False)
    return h


def packed() -> np.ndarray:
    """The fp64 array ``smoltts_limiter_create`` takes: the three phases, one after the other."""
    return np.ascontiguousarray(interpolator().reshape(-1))


def peaks(xp: np.ndarray, n: int) -> np.ndarray:
    """p of ``n`` samples; ``xp``: float64 [n + TAPS - 1], the samples with the 5 in front of them and the 6 behind."""
    h = interpolator()
    p = np.abs(xp[-K_LO: -K_LO + n])
    for q in range(3):
        y = np.zeros(n)
        for k in range(TAPS):
            y = y + h[q, k] * xp[k: k + n]
        p = np.maximum(p, np.abs(y))
    return p


def required(p: np.ndarray, c: float) -> np.ndarray:
    """r of p: c / p where p > c, else 1.0."""
    r = np.ones(p.size)
    over = p > c
    r[over] = np.float64(c) / p[over]
    return r


def sliding_min(a: np.ndarray, w: int) -> np.ndarray:
    """``out[i] = min a[i .. i+w-1]``, a.size - w + 1 values (the minimum is order-free: any decomposition gives these bits)."""
    cur, span = a, 1
    while span * 2 <= w:
        cur = np.minimum(cur[:-span], cur[span:])
        span *= 2
    n = a.size - w + 1
    return np.minimum(cur[:n], cur[w - span: w - span + n])


def smooth(m: np.ndarray, r: np.ndarray) -> np.ndarray:
    """g of ``r.size`` samples; ``m``: float64 [r.size + L], m of the samples and of the L in front of them."""
    n = r.size
    s = np.zeros(n)
    for i in range(MEAN):  # oldest first
        s = s + m[i: i + n]
    return np.minimum(r, s / np.float64(MEAN))


def gains(x: np.ndarray, peak_limit_db: float) -> np.ndarray:
    """g of the whole utterance ``x`` (float64 [n])."""
    xd = np.asarray(x, np.float32).reshape(-1).astype(np.float64)
    n = int(xd.size)
    c = ceiling_of_db(peak_limit_db)
    r = required(peaks(np.concatenate([np.zeros(-K_LO), xd, np.zeros(K_HI)]), n), c)
    m = sliding_min(np.concatenate([np.ones(R), r, np.ones(L)]), WINDOW)
    return smooth(np.concatenate([np.ones(L), m]), r)


def limit(x: np.ndarray, peak_limit_db: float) -> Tuple[np.ndarray, float]:
    """(y, min g) of the whole utterance ``x`` (float32 at 24 kHz): as many samples out as in; min g is 1.0 when nothing was
    limited (and for an empty utterance)."""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
    if x.size == 0:
        return x.copy(), 1.0
    g = gains(x, peak_limit_db)
    return (x.astype(np.float64) * g).astype(np.float32), float(g.min())


class StreamState:
    """The limiter for one stream.  ``process(x, last)`` returns the samples that became final with the call: in total
    ``max(0, fed - HOLD_BACK)`` so far, and everything once ``last`` is set.  What it returns does not depend on how the calls
    cut the stream.  It keeps what the device keeps: the last ``HOLD_BACK`` samples, the last ``R_HIST`` required gains, the
    position, c and the running min g."""

    def __init__(self, peak_limit_db: float = None, ceiling: float = None):
        self.c = np.float64(ceiling_of_db(peak_limit_db) if ceiling is None else ceiling)
        self.pos = 0
        self.ended = False
        self.min_g = np.float64(1.0)
        self.xh = np.zeros(HOLD_BACK, np.float32)  # x[pos - 126 .. pos - 1] (0 before the stream)
        self.rh = np.ones(R_HIST)                  # r[pos - 1446 .. pos - 7] (1 before the stream)

    def process(self, x: np.ndarray, last: bool = False) -> np.ndarray:
        x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
        if self.ended:
            return np.zeros(0, np.float32)
        n, f = int(x.size), self.pos
        nv = n + (HOLD_BACK if last else 0)  # the zeros behind the end push the held samples out
        if nv == 0:
            return np.zeros(0, np.float32)
        xv = np.concatenate([self.xh, x, np.zeros(nv - n, np.float32)]).astype(np.float64)  # x[f - 126 .. f + nv - 1]
        at = f - K_HI + np.arange(nv)  # the positions whose r is new: their last tap has arrived
        r_new = required(peaks(xv[HOLD_BACK - K_HI + K_LO:], nv), self.c)
        r_new[(at < 0) | (last & (at >= f + n))] = 1.0  # outside the stream
        r = np.concatenate([self.rh, r_new])  # r[f - 1446 .. f + nv - 7]
        m = sliding_min(r, WINDOW)            # m[f - 246 .. f + nv - 127]
        m[f - HOLD_BACK - L + np.arange(m.size) < 0] = 1.0  # before the stream
        g = smooth(m, r[R + L: R + L + nv])   # g[f - 126 .. f + nv - 127]
        y = (xv[:nv] * g).astype(np.float32)
        self.min_g = np.minimum(self.min_g, g.min())
        self.rh = r[-R_HIST:].copy()
        self.xh = np.concatenate([self.xh, x])[-HOLD_BACK:].copy()
        self.pos, self.ended = f + n, bool(last)
        return y[max(0, HOLD_BACK - f):]

    def state(self) -> dict:
        """What ``PeakLimiter.slot_state`` reads from the device."""
        return {"pos": int(self.pos), "ended": int(self.ended), "c": float(self.c), "min_g": float(self.min_g),
                "x": self.xh.copy(), "r": self.rh.copy()}
