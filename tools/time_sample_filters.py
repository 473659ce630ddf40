"""Time a sampled frame step of slot mode with the per-request filters (csrc/argmax_dev.h) off, with top_k only and with top_p +
repetition penalty: ``--slots`` requests of the ``--model`` synthetic model, ``--frames`` decode frames per run.  Prints the mean
time per frame from device events; run it under ``rocprofv3 --kernel-trace --stats -- python3 tools/time_sample_filters.py --config K``
(one configuration per run) for the per-launch time of the two picking kernels (argmax_kernel, commit_embed_kernel)."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.config import TokenConfig  # noqa: E402
from smoltts_amd.engine import LMEngine, LMSession  # noqa: E402
from smoltts_amd.prompt import PromptEncoder  # noqa: E402
from smoltts_amd.synthetic import named_config, synthetic_lm_state  # noqa: E402
from smoltts_amd.tokenizer import load_tokenizer  # noqa: E402

CONFIGS = {"off": None, "top_k": (1.0, 50, 1.0, 16), "top_p_penalty": (0.9, 0, 1.2, 16), "all": (0.9, 50, 1.2, 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="smoltts_byte_70m")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS), help="one configuration only (default: all of them in turn)")
    a = ap.parse_args()
    cfg = named_config(a.model)
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=21), tc)
    prompts = [pe.build_prompt(f"request number {b}", "heart") for b in range(a.slots)]
    slots = list(range(a.slots))
    for name in ([a.config] if a.config else list(CONFIGS)):
        s = LMSession(eng, a.slots, max_seq=512, max_rows=128 * a.slots, max_frames=a.frames + 24)
        s.set_slot_sampling(slots, [0.8] * a.slots, [0.8] * a.slots, [0.0] * a.slots, [b + 1 for b in slots])
        if CONFIGS[name] is not None:
            s.set_slot_filters(slots, *[[v] * a.slots for v in CONFIGS[name]])
        s.prefill(prompts, stop_on_eos=False)
        s.decode(20)  # captures the frame graphs
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        s.decode(a.frames)
        t1.record()
        torch.cuda.synchronize()
        print(f"{name}: {a.slots} slots, {a.frames} frames: {1e3 * t0.elapsed_time(t1) / a.frames:.1f} us per frame (events)", flush=True)
        s.close()


if __name__ == "__main__":
    main()
