"""What a forced-alignment call costs: a 10 s recording (125 frames) behind a prompt of 100 columns on the
smoltts_byte_150m synthetic model, two heads in each of two layers, in a one-slot session, the whole grid in one call of the
library.  Device events on the call's stream, median of 10 calls per variant:

    rows prefill          measure_rows with no heads chosen and no targets (what a non-final prefill chunk of the grid costs)
    + alignment launches  heads chosen, no targets
    + head and score      heads chosen, every audio row scored

    python tools/time_forced_align.py [frames] [prompt columns] [max_seq]

``max_seq`` (default: just what the grid needs) is the session's cache length, which sizes the alignment kernel's LDS."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from smoltts_amd.config import NumericsMode, TokenConfig  # noqa: E402
from smoltts_amd.engine import LMEngine, LMSession  # noqa: E402
from smoltts_amd.synthetic import named_config, synthetic_lm_state  # noqa: E402
from smoltts_amd.tokenizer import load_tokenizer  # noqa: E402

PAIRS = [(4, 1), (4, 7), (8, 2), (8, 10)]
RUNS = 10


def timed(s, grid, frames, targets):
    ms = []
    for run in range(RUNS + 1):  # (run 0 warms the kernels)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        it = s.iter_measure_rows(grid, 0, frames, targets)
        try:
            while True:
                next(it)
        except StopIteration:
            pass
        e1.record()
        torch.cuda.synchronize()
        if run:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), ms


def main():
    F = int(sys.argv[1]) if len(sys.argv) > 1 else 125
    T0 = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    cfg = named_config("smoltts_byte_150m")
    tc = TokenConfig.from_tokenizer(load_tokenizer(), cfg)
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=0), tc, NumericsMode.torch_reference())
    rng = np.random.default_rng(0)
    T = T0 + F
    grid = rng.integers(0, cfg.codebook_size, size=(1 + cfg.max_fast_seqlen, T)).astype(np.int32)
    grid[0, :T0] = rng.integers(0, 256, size=T0)
    grid[1:, :T0] = 0
    grid[0, T0:] = grid[1, T0:] + tc.semantic_start_id
    frames = np.full(T, -1, np.int32)
    frames[T0 - 1: T0 - 1 + F] = np.arange(F)
    targets = np.full(T, -1, np.int32)
    targets[T0 - 1:] = grid[0, T0:].tolist() + [tc.im_end_id]
    none = np.full(T, -1, np.int32)
    max_seq = int(sys.argv[3]) if len(sys.argv) > 3 else T + 1
    s = LMSession(eng, 1, max_seq=max_seq, max_rows=T, max_frames=F)
    t_rows, _ = timed(s, grid, frames, none)
    s.set_align_heads(PAIRS)
    s.set_slot_align([0], [10], [T0 - 10])
    t_heads, _ = timed(s, grid, frames, none)
    t_all, runs = timed(s, grid, frames, targets)
    print(f"{F} frames behind {T0} prompt columns ({T} rows), max_seq {max_seq}, {len(PAIRS)} heads in 2 layers, median of {RUNS}:")
    print(f"  rows prefill         {t_rows:8.3f} ms")
    print(f"  alignment launches   {t_heads - t_rows:8.3f} ms  ({(t_heads - t_rows) * 1e3 / (2 * F):.2f} us per measured row and launch)")
    print(f"  head and score       {t_all - t_heads:8.3f} ms  ({(t_all - t_heads) * 1e3 / (F + 1):.2f} us per scored row: a copy, a GEMM and a score launch each)")
    print(f"  the whole call       {t_all:8.3f} ms  (runs: {', '.join(f'{r:.2f}' for r in runs)})")
    s.close()
    eng.close()


if __name__ == "__main__":
    main()
