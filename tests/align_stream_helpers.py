"""Planted alignment rows for the streamed-timestamp tests: float32 ``m`` / ``s1`` [F, H] as the session writes
them, and the numpy model run over them."""
import numpy as np

from smoltts_amd import align


def rows_of(m, cen):
    """Mass ``m`` [F, H] and one centroid per frame ``cen`` [F] -> float32 (m, s1) with s1 = m * centroid per head."""
    m = np.asarray(m, np.float32)
    s1 = (m.astype(np.float64) * np.asarray(cen, np.float64)[:, None]).astype(np.float32)
    return m, s1


def noisy(seed, F=48, H=4, n=17):
    """Noisy centroids around a line over the text; frame 0 is not measured."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.05, 0.5, (F, H))
    cen = np.linspace(0, n - 1, F) + rng.normal(0, 1.5, F)
    m, s1 = rows_of(m, np.clip(cen, 0, n - 1))
    m[0], s1[0] = -1.0, 0.0
    return m, s1


def ramp(F=40, H=2, n=12, outlier=False):
    """The line 0 .. n - 1, lowered by 0.45 at every third frame: pooling stays local.  ``outlier``: frame 30 looks at token 1."""
    m = np.random.default_rng(0).uniform(0.2, 0.6, (F, H))
    cen = np.linspace(0, n - 1, F)
    cen[np.arange(F) % 3 == 2] -= 0.45
    if outlier:
        cen[30] = 1.0
    return rows_of(m, cen)


def gaps(F=40, H=2, n=12):
    """The ramp with frame 0 not measured and four frames below MIN_MASS."""
    m, s1 = ramp(F, H, n)
    m[0], s1[0] = -1.0, 0.0
    for f in (5, 6, 17, 33):
        m[f] = np.float32(0.01 / H)
        s1[f] = m[f] * np.float32(3.0)
    return m, s1


def weightless(F=40, H=2):
    m = np.full((F, H), 0.001, np.float32)
    return m, (m * np.float32(2.0)).astype(np.float32)


def model_trace(m, s1, n, lag, F=None):
    """The model pushed frame by frame and finished at ``F`` (default: every frame): (starts after each frame as a list of
    arrays, the final starts)."""
    sf = align.StreamFit(n, lag)
    trace = []
    for f in range(m.shape[0]):
        sf.push(m[f], s1[f])
        trace.append(np.asarray(sf.starts, np.float64))
    return trace, sf.finish(m.shape[0] if F is None else F)
