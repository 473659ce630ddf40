"""Cloned-voice prefixes at serving scale: smoltts_byte_150m shapes (seeded weights), B = 32, a voice of about
10 s of audio (125 audio columns + its transcript and turn tokens).

  --mode install   install launches of the voice's prefix into 1 and into 8 slots, nothing else: run it under
                   `rocprofv3 --kernel-trace --stats -- python tools/time_voice_prefix.py --mode install` for the kernel times
  --mode arrival   time to frame 0 of one cloned-voice arrival among 31 speaking slots, and the frames/s those 31 slots deliver
                   meanwhile, both ways, alternating:
                     cached    the prefix installed + the request's own turns prefilled on the side path (what the scheduler does)
                     uncached  the whole prompt (speaker turns included) prefilled in line in chunks of 128 with a tick between
                   (the scheduler has no uncached path: emulated on the LMSession the way BatchScheduler drives it)

Timing: device events on the frame stream, from the arrival's first launch to the end of the frame that emits its frame 0; the
host waits of the side path fall inside that span.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TICK = 4
CHUNK = 128
TRANSCRIPT = ("This is a reference recording of about ten seconds, read slowly and clearly so that the model can pick up the "
              "speaker's voice.")


def setup(name: str, kv: str):
    from smoltts_amd.config import TokenConfig
    from smoltts_amd.engine import LMEngine, LMSession
    from smoltts_amd.prompt import PromptEncoder
    from smoltts_amd.synthetic import named_config, synthetic_lm_state
    from smoltts_amd.tokenizer import load_tokenizer

    cfg = named_config(name)
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=3), tc)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    codes = np.random.default_rng(1).integers(0, cfg.codebook_size, size=(cfg.num_codebooks, 125))
    grid = np.concatenate([pe.encode_text_turn("user", TRANSCRIPT), pe.encode_vq(codes)], axis=1).astype(np.int32)
    scratch = LMSession(eng, 1, max_seq=cfg.max_seq_len, max_rows=CHUNK, max_frames=1, kv_dtype=kv)
    for a in range(0, grid.shape[1], CHUNK):
        scratch.prefill([grid[:, a: a + CHUNK]], [0], pos0=[a], final=False)
    pk = scratch.save_prefix(0, grid.shape[1])
    torch.cuda.synchronize()
    scratch.close()
    return cfg, eng, pe, grid, pk


def mode_install(args) -> dict:
    from smoltts_amd.engine import LMSession

    cfg, eng, pe, grid, pk = setup(args.model, args.kv)
    s = LMSession(eng, args.batch, max_seq=cfg.max_seq_len, max_rows=512, max_frames=8, kv_dtype=args.kv)
    for n in (1, 8):
        for _ in range(args.reps):
            s.install_prefix([pk] * n, list(range(n)))
    torch.cuda.synchronize()
    s.close()
    return {"mode": "install", "P": pk.n_positions, "prefix_bytes": pk.nbytes - 256, "reps": args.reps,
            "launches": {"1_slot": args.reps, "8_slots": args.reps}}


def mode_arrival(args) -> dict:
    from smoltts_amd.engine import LMSession

    cfg, eng, pe, grid, pk = setup(args.model, args.kv)
    P = grid.shape[1]
    B = args.batch
    s = LMSession(eng, B, max_seq=cfg.max_seq_len, max_rows=2048, max_frames=1025, kv_dtype=args.kv)
    s.set_frames_per_graph(TICK)
    voices = ["heart", "bella", "nova", "sky", "sarah", "michael", "fenrir", "liam"]
    speakers = [pe.build_prompt(f"speaking slot number {b} keeps talking", voices[b % len(voices)]) for b in range(B - 1)]
    s.prefill(speakers, slots=list(range(B - 1)), stop_on_eos=False, defer_frame0=True)
    full = pe.build_prompt("hello, this request asks for the cloned voice", "cv", grid)
    suffix = full[:, P:]
    frames = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    arrival = B - 1
    for _ in range(4):  # warm-up: graphs captured, every path run once
        s.decode(TICK)
    res = {"cached": [], "uncached": []}
    fps = {"cached": [], "uncached": []}

    def one(kind: str) -> None:
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(frames)
        n_frames = 0
        if kind == "cached":
            h = s.side_park([suffix], [arrival], prefixes=[pk])
            s.decode(TICK)  # the tick the side call runs beside
            n_frames += TICK
            with torch.cuda.stream(side):
                s.side_run(h)
            s.side_start(h, stop_on_eos=False)
        else:
            def between():
                nonlocal n_frames
                s.decode(TICK)
                n_frames += TICK

            s.prefill_chunked([full], slots=[arrival], stop_on_eos=False, chunk=CHUNK, between=between, defer_frame0=True)
        s.decode(1)  # the frame that emits the arrival's frame 0
        n_frames += 1
        ev1.record(frames)
        s.decode(TICK - 1)
        torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1)
        res[kind].append(ms)
        fps[kind].append((B - 1) * n_frames / (ms / 1e3))

    for i in range(args.reps):
        for kind in (("cached", "uncached") if i % 2 == 0 else ("uncached", "cached")):
            one(kind)
    s.close()

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}

    return {"mode": "arrival", "model": args.model, "B": B, "P": P, "suffix_T": int(suffix.shape[1]), "prefix_bytes": pk.nbytes - 256,
            "ms_to_frame0": {k: summary(v) for k, v in res.items()},
            "speaking_frames_per_s": {k: summary(v) for k, v in fps.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["install", "arrival"], required=True)
    ap.add_argument("--model", default="smoltts_byte_150m")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kv", default="fp32")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    out = mode_install(args) if args.mode == "install" else mode_arrival(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
