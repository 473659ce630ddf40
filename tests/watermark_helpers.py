"""Seeded speech-like test signals for the watermark tests, and the channels a marked signal goes through.

``speechlike(seed, seconds)``: syllables of 120-300 ms with gaps of 40-160 ms between them.  Three syllables in four are voiced:
a harmonic source (f0 90-220 Hz with a 5 Hz vibrato of 3 %, harmonics falling by 1/k up to 5 kHz) through four formant
resonators (two-pole filters at seeded centre frequencies around 600, 1500, 2600 and 3600 Hz), under a raised-cosine syllable
envelope.  The others are unvoiced: a fricative burst of white noise high-passed around 2.5-5 kHz.  A breath of noise at -50 dB
lies under everything, the peak is scaled to a seeded level between 0.2 and 0.8, and the result is float32 at 24 kHz."""
import numpy as np
from scipy.signal import butter, lfilter, resample_poly

FS = 24000


def speechlike(seed: int, seconds: float = 2.0) -> np.ndarray:
    rng = np.random.default_rng([seed, 0x57A7])
    n = int(round(seconds * FS))
    x = np.zeros(n)
    at = int(rng.uniform(0.0, 0.05) * FS)
    while at < n:
        ln = int(rng.uniform(0.12, 0.30) * FS)
        m = min(ln, n - at)
        t = np.arange(ln) / FS
        env = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(ln) / ln)
        if rng.uniform() < 0.75:
            f0 = rng.uniform(90.0, 220.0) * (1.0 + 0.03 * np.sin(2.0 * np.pi * 5.0 * t + rng.uniform(0, 6.28)))
            ph = 2.0 * np.pi * np.cumsum(f0) / FS
            src = np.zeros(ln)
            for k in range(1, int(5000.0 / 220.0) + 1):
                src += np.sin(k * ph) / k
            seg = np.zeros(ln)
            for fc, bw, amp in zip((600.0, 1500.0, 2600.0, 3600.0), (80.0, 110.0, 160.0, 200.0), (1.0, 0.6, 0.3, 0.15)):
                fc = fc * rng.uniform(0.75, 1.3)
                r = np.exp(-np.pi * bw / FS)
                a = [1.0, -2.0 * r * np.cos(2.0 * np.pi * fc / FS), r * r]
                seg += amp * lfilter([1.0 - r], a, src)
            seg = seg / np.max(np.abs(seg))
        else:
            b, a = butter(2, rng.uniform(2500.0, 5000.0) / (FS / 2), "high")
            seg = 0.3 * lfilter(b, a, rng.standard_normal(ln))
            seg = seg / np.max(np.abs(seg)) * 0.4
        x[at: at + m] += (rng.uniform(0.4, 1.0) * env * seg)[:m]
        at += ln + int(rng.uniform(0.04, 0.16) * FS)
    x += 10.0 ** (-50.0 / 20.0) * rng.standard_normal(n)
    return (x / np.max(np.abs(x)) * rng.uniform(0.2, 0.8)).astype(np.float32)


def to_int16(x: np.ndarray) -> np.ndarray:
    """The blocking route's 16-bit samples."""
    return np.rint(np.clip(np.asarray(x, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)


def through_rate(x: np.ndarray, rate: int) -> np.ndarray:
    """``pcm_<rate>`` as a receiver has it: resampled from 24 kHz (scipy's default filter, which the resampler stage
    reproduces), rounded to int16."""
    from math import gcd

    g = gcd(FS, rate)
    return to_int16(resample_poly(np.asarray(x, np.float64), rate // g, FS // g))


def ulaw_decode(b: np.ndarray) -> np.ndarray:
    """G.711 mu-law bytes -> int16 (the inverse of ``formats.lin2ulaw`` up to its quantisation)."""
    u = ~np.asarray(b, np.uint8) & 0xFF
    mag = ((((u & 0x0F).astype(np.int32) << 3) + 0x84) << ((u >> 4) & 7).astype(np.int32)) - 0x84
    return np.where(u & 0x80, -mag, mag).astype(np.int16)
