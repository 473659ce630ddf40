"""What the alignment rows cost a decode frame: frames/s of the smoltts_byte_150m synthetic model at B = 32, greedy,
with two heads in each of two layers measured for every slot, against the option off, alternating in one session.

    python tools/bench_align.py [frames per run] [runs] [max_seq]
    python tools/bench_align.py --live [frames per run] [runs]      (streamed timestamps, DESIGN.md 24: see live_main)

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


def live_main(frames: int, runs: int, tick: int = 4, lag: int = 6):
    """``--live``: frames/s in ticks of four frames with what the scheduler queues behind each tick -- the clones of
    the output ring, and with the option off nothing else; with blocking timestamps the clone of the row buffer; with live
    timestamps the fit kernel and the clones of its counts and starts -- alternating in one session; then the fit kernel's time
    per call beside the numpy model's time per pushed frame over the same rows."""
    import time

    from smoltts_amd.align import StreamFit
    from smoltts_amd.lm import AlignFitter

    cfg = named_config("smoltts_byte_150m")
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=0), TokenConfig.from_tokenizer(load_tokenizer(), cfg), NumericsMode.torch_reference())
    rng = np.random.default_rng(0)
    prompts = []
    for _ in range(B):
        g = rng.integers(0, cfg.codebook_size, size=(1 + cfg.max_fast_seqlen, T)).astype(np.int32)
        g[0] = rng.integers(0, 256, size=T)
        g[1] = np.maximum(g[1], 1)
        prompts.append(g)
    s = LMSession(eng, B, max_seq=T + frames + 8, max_rows=B * T, max_frames=frames + 1)
    s.set_frames_per_graph(tick)
    s.set_slot_sampling(list(range(B)), [0.0] * B, [0.0] * B, [0.0] * B, [0] * B)
    s.set_align_heads(PAIRS)
    fit = AlignFitter.for_session(s)
    n_tok = T - 20
    rates = {"off": [], "blocking": [], "live": []}
    for run in range(runs + 1):  # (run 0 captures the graphs of both forms)
        for mode in rates:
            on = mode != "off"
            s.set_slot_align(list(range(B)), [10] * B, [T - 10 if on else 10] * B)
            s.prefill(prompts, stop_on_eos=False, defer_frame0=True)
            fit.reset_slots(list(range(B)), [n_tok if mode == "live" else None] * B, [lag] * B, [frames] * B)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(frames // tick):
                s.decode(tick)
                keep = [s.codes.clone(), s.n_frames.clone(), s.done.clone()]
                if mode == "blocking":
                    keep.append(s.alignment.clone())
                elif mode == "live":
                    fit.push(s.alignment, s.n_frames, s.done)
                    keep += [fit.committed.clone(), fit.starts[:, :n_tok].clone()]
            e1.record()
            torch.cuda.synchronize()
            if run:
                rates[mode].append(B * frames / (e0.elapsed_time(e1) / 1e3))
    off = np.median(rates["off"])
    for mode, r in rates.items():
        print(f"timestamps {mode:8s}: {np.median(r):.0f} frames/s (costs {100 * (off - np.median(r)) / off:.2f} % of off; runs: {', '.join(f'{x:.0f}' for x in r)})")
    # the fit alone: the last run's rows, the counters stepped a tick at a time
    rows = s.alignment
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    fit.reset_slots(list(range(B)), [n_tok] * B, [lag] * B, [frames] * B)
    us = []
    for f in range(tick, frames + 1, tick):
        counts.fill_(f)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fit.push(rows, counts, done)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    print(f"fit kernel: {np.median(us):.1f} us per call (median of {len(us)}; max {max(us):.1f}) for {B} slots x {tick} frames, events around the launch")
    host = rows.cpu().numpy()
    t0 = time.perf_counter()
    for b in range(B):
        sf = StreamFit(n_tok, lag)
        for f in range(frames):
            sf.push(host[b, f, :, 0], host[b, f, :, 1])
    dt = time.perf_counter() - t0
    print(f"numpy model: {1e6 * dt / (B * frames):.1f} us per pushed frame on the host = {1e6 * dt / (B * frames) * B * tick:.0f} us per tick of {B} slots x {tick} frames")
    fit.close()
    s.close()
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--live":
        live_main(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    else:
        main()
