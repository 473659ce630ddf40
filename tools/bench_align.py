"""What the alignment rows cost a decode frame: frames/s of the smoltts_byte_150m synthetic model at B = 32, greedy,
with two heads in each of two layers measured for every slot, against the option off, alternating in one session.

    python tools/bench_align.py [frames per run] [runs] [max_seq]

``max_seq`` (default: just what the run needs) is the session's cache length, which sizes the kernel's LDS.

Every run decodes the same number of frames from the same prompts (the slots are prefilled anew, stop_on_eos off), in four-frame
graphs; the time is taken by events around the decode call."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from smoltts_amd.config import NumericsMode, TokenConfig  # noqa: E402
from smoltts_amd.engine import LMEngine, LMSession  # noqa: E402
from smoltts_amd.synthetic import named_config, synthetic_lm_state  # noqa: E402
from smoltts_amd.tokenizer import load_tokenizer  # noqa: E402

B, T = 32, 120
PAIRS = [(4, 1), (4, 7), (8, 2), (8, 10)]


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cfg = named_config("smoltts_byte_150m")
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=0), TokenConfig.from_tokenizer(load_tokenizer(), cfg), NumericsMode.torch_reference())
    rng = np.random.default_rng(0)
    prompts = []
    for _ in range(B):
        g = rng.integers(0, cfg.codebook_size, size=(1 + cfg.max_fast_seqlen, T)).astype(np.int32)
        g[0] = rng.integers(0, 256, size=T)
        g[1] = np.maximum(g[1], 1)
        prompts.append(g)
    max_seq = int(sys.argv[3]) if len(sys.argv) > 3 else T + frames + 8
    s = LMSession(eng, B, max_seq=max_seq, max_rows=B * T, max_frames=frames + 1)
    s.set_frames_per_graph(4)
    s.set_slot_sampling(list(range(B)), [0.0] * B, [0.0] * B, [0.0] * B, [0] * B)
    s.set_align_heads(PAIRS)
    rates = {False: [], True: []}
    for run in range(runs + 1):  # (run 0 captures the graphs of both forms)
        for on in (False, True):
            s.set_slot_align(list(range(B)), [10] * B, [T - 10 if on else 10] * B)
            assert bool(s.graph_form() & 32) == on
            s.prefill(prompts, stop_on_eos=False, defer_frame0=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.decode(frames)
            e1.record()
            torch.cuda.synchronize()
            if run:
                rates[on].append(B * frames / (e0.elapsed_time(e1) / 1e3))
    for on in (False, True):
        print(f"alignment {'on ' if on else 'off'}: {np.median(rates[on]):.0f} frames/s (runs: {', '.join(f'{r:.0f}' for r in rates[on])})")
    off, on = np.median(rates[False]), np.median(rates[True])
    print(f"cost: {100 * (off - on) / off:.2f} % of the frame rate for {len(PAIRS)} heads in 2 layers (2 launches per frame), max_seq {max_seq}")
    s.close()
    eng.close()


if __name__ == "__main__":
    main()
