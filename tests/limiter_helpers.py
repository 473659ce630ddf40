"""Signals and small tools the limiter tests share: the watermark tests' speech-like signals driven into the ceiling, an isolated
impulse in noise, the model run over a list of cuts, and an independent 8x reading of a signal's peak."""
from functools import lru_cache

import numpy as np

from smoltts_amd import limiter as LM

from watermark_helpers import speechlike

SEEDS = tuple(range(12))
DRIVES_DB = (0.0, 6.0, 12.0)
CEILINGS_DB = (0.0, -1.0, -6.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@lru_cache(maxsize=None)
def _speech(seed: int, seconds: float) -> np.ndarray:
    x = speechlike(seed, seconds)
    x.setflags(write=False)
    return x


def driven(seed: int, drive_db: float = 0.0, seconds: float = 2.0) -> np.ndarray:
    """``speechlike(seed, seconds)`` raised by ``drive_db`` (float32, computed in float64)."""
    return (_speech(seed, seconds).astype(np.float64) * 10.0 ** (drive_db / 20.0)).astype(np.float32)


def impulse(n: int = 6000, at: int = 3000, height: float = 2.0, seed: int = 5) -> np.ndarray:
    """One sample of ``height`` in uniform noise of amplitude 2^-10."""
    x = (np.random.default_rng(seed).uniform(-1.0, 1.0, n) * 2.0 ** -10).astype(np.float32)
    x[at] = height
    return x


def stream(x: np.ndarray, peak_limit_db: float, cuts, last_empty: bool = False):
    """(the model's stream output over ``cuts``, a list of call lengths that the rest of ``x`` follows in one last call (alone in
    an empty call behind it with ``last_empty``); the samples each call returned; the state at the end)."""
    st, out, at = LM.StreamState(peak_limit_db), [], 0
    for c in cuts:
        out.append(st.process(x[at: at + c]))
        at += min(c, x.size - at)
    if last_empty:
        out.append(st.process(x[at:]))
        out.append(st.process(x[:0], last=True))
    else:
        out.append(st.process(x[at:], last=True))
    return np.concatenate(out), [o.size for o in out], st


def peak_8x(y: np.ndarray) -> float:
    """max |y| after an 8x ``scipy.signal.resample_poly``: a reading that does not use the stage's own interpolator."""
    from scipy.signal import resample_poly

    return float(np.abs(resample_poly(np.asarray(y, np.float64), 8, 1)).max())
