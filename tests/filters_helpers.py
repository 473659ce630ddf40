"""The rows of the sampling-filter tests (top_k / top_p / repetition penalty), shared by the CPU check of the fixture seeds and
the GPU kernel test: 64 rows per shape with the options spread over them."""
import numpy as np

R = 64
SHAPES = (2048, 1001)  # the vector path and the scalar path (n_cols % 4 != 0) of the pick
STEPS = (0, 3)
TEMPS = [0.0, 0.3, 0.7, 1.0, 1.5, 0.9, 2.0, 0.6]
FASTS = [0.5, 0.0, 1.2, 0.9, 0.8, 0.4, 0.0, 1.0]
MIN_PS = [0.0, 0.0, 0.05, 0.2]


def configs(V):
    """(top_k, top_p, penalty, history length, window) of row r = entry r % 16: each filter alone and all together."""
    return [(0, 1.0, 1.0, 0, 64), (1, 1.0, 1.0, 0, 64), (2, 1.0, 1.0, 0, 64), (50, 1.0, 1.0, 0, 64), (V, 1.0, 1.0, 0, 64),
            (0, 1e-6, 1.0, 0, 64), (0, 0.5, 1.0, 0, 64), (0, 0.9, 1.0, 0, 64), (0, 1.0, 1.2, 1, 64), (0, 1.0, 3.0, 16, 64),
            (0, 1.0, 1.2, 64, 64), (50, 0.9, 1.2, 16, 64), (2, 0.5, 3.0, 64, 4), (50, 0.5, 1.0, 0, 64), (0, 0.9, 3.0, 1, 16),
            (V, 1e-6, 1.2, 0, 64)]


def make_rows(V, seed=None):
    """dict of the fixture of shape V: logits [R, V] float32 (randn * 3), per-row options, history [R, 64] int32 (newest
    first, with duplicates, the row's largest columns among them so that the penalty moves the pick) and seeds."""
    rng = np.random.default_rng(1000 + V if seed is None else seed)
    logits = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)
    cfg = configs(V)
    rows = [cfg[r % 16] for r in range(R)]
    hist = np.zeros((R, 64), np.int32)
    for r in range(R):
        top = np.argsort(-logits[r])[:24]
        h = np.concatenate([top[:1], rng.permutation(np.concatenate([top[1:], rng.integers(0, V, 40)]))]).astype(np.int32)
        h[5], h[63] = h[0], h[2]  # duplicates
        hist[r] = h
    return dict(
        V=V, logits=logits, top_k=[c[0] for c in rows], top_p=[c[1] for c in rows], penalty=[c[2] for c in rows],
        hist_len=[c[3] for c in rows], window=[c[4] for c in rows], history=hist,
        temps=[TEMPS[(r + r // 16) % 8] for r in range(R)], fasts=[FASTS[(r + r // 16) % 8] for r in range(R)],
        min_ps=[MIN_PS[(r // 3) % 4] for r in range(R)], seeds=[int(x) for x in rng.integers(0, 2**63, R)],
        frames=[3 * r + 1 for r in range(R)])


def row_args(fx, r, step):
    """Keyword arguments of sampling.filtered_pick / filtered_keys / top_p_edge's filter part for row r."""
    n = min(fx["hist_len"][r], fx["window"][r])
    return dict(top_k=fx["top_k"][r], top_p=fx["top_p"][r], penalty=fx["penalty"][r], history=fx["history"][r][:n])


def row_temp(fx, r, step):
    return (fx["temps"] if step == 0 else fx["fasts"])[r]
