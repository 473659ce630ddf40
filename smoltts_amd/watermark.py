"""A keyed spread-spectrum watermark for 24 kHz mono speech: the numpy model that defines what ``csrc/watermark.hip`` computes
(DESIGN.md section 17), and the detector.  The device reproduces the embedder bit for bit: every fp64 operation below is a
single rounded multiply, add, divide or square root in a fixed order, the chip table and the shaping filter are computed here
and uploaded, and nothing depends on how calls cut the stream.

Grid: blocks of ``L`` = 480 samples (20 ms), counted from the first sample the stage sees of a stream; the chip sequence
repeats every ``P`` = 32 blocks (``PERIOD`` = 15360 samples, 0.64 s).

Chips: ``c[i]`` in {+1, -1} for i < PERIOD, +1 where the top bit of ``splitmix64(key ^ (i * 0xD1342543DE82EF95))`` is set (all
arithmetic 64-bit wrapping; the finaliser adds 0x9E3779B97F4A7C15, then z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
z *= 0x94D049BB133111EB, z ^= z >> 31).  The chip of sample n is ``c[n mod PERIOD]``.

Shaping filter: ``h`` = (lp(3400 Hz) - lp(500 Hz)) * hamming(65) with lp(fc)[k] = 2 fc / R * sinc(2 fc / R * (k - 32)), scaled to
unit energy, fp64: the mark lives in the telephone band.

Envelope: E_j = the sum of x^2 over block j in fp64, as sequential sums over sub-blocks of ``SUB`` = 16 samples on the stream's
grid, folded sequentially over the block's 30 sub-blocks.  g_j = a * sqrt(E_{j-1} / 480), g_0 = 0, a = 10^(strength_db / 20):
block j's gain uses only the block in front of it, so a slot emits exactly the samples it reads and holds nothing back.

Output: u[n] = g_{n div 480} * c[n mod PERIOD] (0 for n < 0), w[n] = sum_{k=0..64} h[k] * u[n-k] in ascending k,
y[n] = float32(double(x[n]) + w[n]).

``strength_db`` ranges over [-40, -20], default -26.  These values, L, P, the band and the detector's threshold are
specification, not measurements, and live here only.  One key per stage (the table is uploaded when the stage is created);
there is no payload: an operator who wants ids derives one key per id and tests the candidates (``detect`` takes a list).

Detector (``detect``; host only): resample to 24 kHz, filter with ``h`` (it is symmetric: the matched filter) and drop the first
64 samples, divide by the RMS of a sliding 480-sample window, fold modulo PERIOD, correlate circularly with the chip table by
FFT, and score the peak against the 15360 offsets' median and MAD: ``score = (peak - median) / (1.4826 MAD)``,
``detected = score >= THRESHOLD``.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np

FS = 24000
L = 480                    # block (20 ms)
P = 32                     # blocks per chip period
PERIOD = L * P             # 15360 samples, 0.64 s
SUB = 16                   # envelope sub-block (divides L)
TAPS = 65
BAND = (500.0, 3400.0)     # Hz
STRENGTH_MIN, STRENGTH_MAX, STRENGTH_DEFAULT = -40.0, -20.0, -26.0
THRESHOLD = 6.0
EPS = 1e-9                 # added to the detector's sliding RMS

_M64 = (1 << 64) - 1
_STRIDE = 0xD1342543DE82EF95


def splitmix64(z: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser of uint64 ``z`` (wrapping)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def check_key(key) -> int:
    """``key`` as a 64-bit integer: an int in [0, 2^64) or a string of 1 to 16 hex digits; ``ValueError`` otherwise."""
    if isinstance(key, str):
        s = key.strip()
        if not 1 <= len(s) <= 16 or any(ch not in "0123456789abcdefABCDEF" for ch in s):
            raise ValueError("watermark key must be 1 to 16 hex digits")
        return int(s, 16)
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) <= _M64:
        raise ValueError("watermark key must be a 64-bit unsigned integer or 1 to 16 hex digits")
    return int(key)


def check_strength(db, what: str = "watermark strength_db") -> float:
    """``db`` as a float; ``ValueError`` outside [-40, -20]."""
    if isinstance(db, bool) or not isinstance(db, (int, float)) or not np.isfinite(db):
        raise ValueError(f"{what} must be a number of dB between {STRENGTH_MIN:g} and {STRENGTH_MAX:g}")
    if not STRENGTH_MIN <= db <= STRENGTH_MAX:
        raise ValueError(f"{what} {db:g} outside [{STRENGTH_MIN:g}, {STRENGTH_MAX:g}] dB")
    return float(db)


@lru_cache(maxsize=64)
def chips(key: int) -> np.ndarray:
    """The chip table of ``key``: float64 [PERIOD] of +1 / -1 (read-only)."""
    with np.errstate(over="ignore"):
        z = np.uint64(check_key(key)) ^ (np.arange(PERIOD, dtype=np.uint64) * np.uint64(_STRIDE))
    c = np.where(splitmix64(z) >> np.uint64(63) != 0, 1.0, -1.0)
    c.setflags(write=False)
    return c


@lru_cache(maxsize=1)
def shaping_filter() -> np.ndarray:
    """``h``: float64 [TAPS], unit energy (read-only)."""
    k = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) // 2

    def lp(fc):
        return 2.0 * fc / FS * np.sinc(2.0 * fc / FS * k)

    h = (lp(BAND[1]) - lp(BAND[0])) * np.hamming(TAPS)
    h = h / np.sqrt(np.sum(h * h))
    h.setflags(write=False)
    return h


def gain_of_db(strength_db: float) -> float:
    """a = 10^(strength_db / 20)."""
    return float(10.0 ** (float(strength_db) / 20.0))


@dataclass(frozen=True)
class Watermark:
    """A key and a strength: what ``SmolTTS``, ``BatchScheduler`` and ``GpuPool`` take as ``watermark``."""
    key: int
    strength_db: float = STRENGTH_DEFAULT

    def __post_init__(self):
        object.__setattr__(self, "key", check_key(self.key))
        object.__setattr__(self, "strength_db", check_strength(self.strength_db))

    def __repr__(self) -> str:  # (the key stays out of logs)
        return f"Watermark(key=<hidden>, strength_db={self.strength_db:g})"

    @property
    def gain(self) -> float:
        return gain_of_db(self.strength_db)

    def packed(self) -> np.ndarray:
        """The fp64 array ``smoltts_watermark_create`` takes: ``h``, then the chip table."""
        return np.concatenate([shaping_filter(), chips(self.key)])


class StreamState:
    """The embedder for one stream.  ``process`` returns exactly as many samples as it is given, and what it returns does not
    depend on how the calls cut the stream."""

    def __init__(self, wm: Watermark, gain: Optional[float] = None):
        self.c, self.h = chips(wm.key), shaping_filter()
        self.a = np.float64(wm.gain if gain is None else gain)
        self.pos = 0
        self.e_sub = np.float64(0.0)   # sum of x^2 over the open sub-block so far
        self.e_blk = np.float64(0.0)   # the open block's complete sub-blocks, folded
        self.g_cur = np.float64(0.0)   # gain of block pos div L
        self.g_prev = np.float64(0.0)  # gain of the block in front of it

    def process(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1))
        n = int(x.size)
        if n == 0:
            return x.copy()
        xd = x.astype(np.float64)
        pos0, r = self.pos, self.pos % SUB
        # sub-block sums: sample after sample inside each sub-block of the stream's grid (the first goes on from e_sub)
        npc = -(-(r + n) // SUB)
        sq = np.zeros(npc * SUB)
        sq[r: r + n] = xd * xd
        sq = sq.reshape(npc, SUB)
        e = np.zeros(npc)
        e[0] = self.e_sub if r else 0.0
        for j in range(SUB):
            e = e + sq[:, j]
        # the walk over the sub-blocks: blocks complete, each sets the gain of the block behind it
        gains = [self.g_prev, self.g_cur]  # of blocks pos0 div L - 1, pos0 div L, ...
        for i in range(npc):
            end = (i + 1) * SUB - r
            if end > n:  # the open sub-block
                self.e_sub = e[i]
                self.pos = pos0 + n
                break
            self.e_blk = self.e_blk + e[i]
            self.e_sub = np.float64(0.0)
            self.pos = pos0 + end
            if self.pos % L == 0:
                self.g_prev, self.g_cur = self.g_cur, self.a * np.sqrt(self.e_blk / np.float64(L))
                self.e_blk = np.float64(0.0)
                gains.append(self.g_cur)
        # u over [pos0 - (TAPS - 1), pos0 + n)
        at = pos0 - (TAPS - 1) + np.arange(n + TAPS - 1, dtype=np.int64)
        u = np.asarray(gains, np.float64)[at // L - (pos0 // L - 1)] * self.c[at % PERIOD]
        w = np.zeros(n)
        for k in range(TAPS):
            w = w + self.h[k] * u[TAPS - 1 - k: TAPS - 1 - k + n]
        return (xd + w).astype(np.float32)

    def state(self) -> dict:
        """What ``Watermarker.slot_state`` reads from the device."""
        return {"pos": int(self.pos), "values": np.array([self.e_sub, self.e_blk, self.g_cur, self.g_prev, self.a], np.float64)}


def embed(x: np.ndarray, wm: Watermark) -> np.ndarray:
    """A whole utterance marked from position 0: the samples a stream gives."""
    return StreamState(wm).process(x)


# ------------------------------------------------------------------------------- detection
class Detection(NamedTuple):
    score: float
    offset: int      # the stream position modulo PERIOD of the input's first sample at the peak
    detected: bool


def _detect_one(z: np.ndarray, key: int) -> Detection:
    f = np.fft.rfft(z)
    corr = np.fft.irfft(f * np.conj(np.fft.rfft(chips(key))), PERIOD)  # corr[d] = sum_i z[i] c[(i - d) mod PERIOD]
    med = np.median(corr)
    mad = np.median(np.abs(corr - med))
    if not mad > 0 or not np.isfinite(mad):
        return Detection(0.0, 0, False)
    d = int(np.argmax(corr))
    score = float((corr[d] - med) / (1.4826 * mad))
    return Detection(score, (PERIOD - d) % PERIOD, bool(score >= THRESHOLD))


def detect(pcm: np.ndarray, key: Union[int, str, Sequence[Union[int, str]]], rate: int = FS):
    """Whether ``pcm`` (mono; floats, or int16 taken as is: the score does not depend on the scale) carries the mark of
    ``key``: a ``Detection``, or a list of them for a list of keys.  Silence, or any input that folds to a constant, scores
    exactly 0.0."""
    from scipy.signal import lfilter, resample_poly

    many = not isinstance(key, (int, np.integer, str))
    keys = [check_key(k) for k in (key if many else [key])]
    x = np.asarray(pcm, np.float64).reshape(-1)
    if int(rate) != FS and x.size:
        from math import gcd

        g = gcd(FS, int(rate))
        x = resample_poly(x, FS // g, int(rate) // g)
    z = np.zeros(PERIOD)
    if x.size >= TAPS and np.all(np.isfinite(x)) and np.any(x != 0):
        x = x / np.max(np.abs(x))  # (keeps EPS relative; the score is scale-free past this)
        m = lfilter(shaping_filter(), 1.0, x)[TAPS - 1:]
        cs = np.concatenate([[0.0], np.cumsum(m * m)])
        i = np.arange(m.size)
        lo, hi = np.maximum(i - L // 2, 0), np.minimum(i + L // 2, m.size)
        m = m / (np.sqrt((cs[hi] - cs[lo]) / L) + EPS)
        m = np.concatenate([m, np.zeros(-m.size % PERIOD)])
        z = m.reshape(-1, PERIOD).sum(axis=0)
    out = [_detect_one(z, k) for k in keys]
    return out if many else out[0]


def main(argv=None) -> int:
    """``python -m smoltts_amd.watermark detect file.wav --key HEX``: prints the score, exit status 0 when detected, 1 when not."""
    import argparse

    ap = argparse.ArgumentParser(prog="python -m smoltts_amd.watermark")
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("detect", help="test a WAV file for the mark of a key")
    d.add_argument("file")
    d.add_argument("--key", required=True, help="the key as up to 16 hex digits")
    a = ap.parse_args(argv)
    from .server.voices import parse_wav

    with open(a.file, "rb") as f:
        pcm, rate = parse_wav(f.read())
    r = detect(pcm, check_key(a.key), rate)
    print(f"detected={str(r.detected).lower()} score={r.score:.2f}")
    return 0 if r.detected else 1


if __name__ == "__main__":
    raise SystemExit(main())
