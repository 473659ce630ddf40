"""Time a frame step of slot mode in the forms the slow-token score touches: ``--slots`` requests of the ``--model``
synthetic model, ``--frames`` decode frames per run, ``--runs`` runs per form, mean time per frame from device events.

  greedy        every slot greedy, nothing scored: the default form (the slow token comes from the head GEMM's tile candidates)
  slow_sampled  slot 0 samples its slow token, depth codes greedy: the slow pick reads the rows of logits (``argmax_row``)
  score_on      every slot greedy, slot 0 scored (bit 4 of the form): the same pick with the SCORE instantiation

``--form`` runs one of them; the first two need no ``set_slot_score``, so the script also runs on a commit without it."""
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

FORMS = ("greedy", "slow_sampled", "score_on")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="smoltts_byte_150m")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--form", default=None, choices=FORMS, help="one form only (default: all of them in turn)")
    a = ap.parse_args()
    cfg = named_config(a.model)
    tok = load_tokenizer()
    tc = TokenConfig.from_tokenizer(tok, cfg)
    pe = PromptEncoder(tok, tc.semantic_start_id, cfg.num_codebooks, cfg.duplicate_code_0)
    eng = LMEngine(cfg, synthetic_lm_state(cfg, seed=21), tc)
    prompts = [pe.build_prompt(f"request number {b}", "heart") for b in range(a.slots)]
    slots = list(range(a.slots))
    for name in ([a.form] if a.form else list(FORMS)):
        times = []
        for _ in range(a.runs):
            s = LMSession(eng, a.slots, max_seq=512, max_rows=128 * a.slots, max_frames=a.frames + 24)
            temps = [0.7 if (name == "slow_sampled" and b == 0) else 0.0 for b in slots]
            s.set_slot_sampling(slots, temps, [0.0] * a.slots, [0.0] * a.slots, [b + 1 for b in slots])
            if name == "score_on":
                s.set_slot_score([0], [True])
            s.prefill(prompts, stop_on_eos=False)
            s.decode(20)  # captures the frame graphs
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            s.decode(a.frames)
            t1.record()
            torch.cuda.synchronize()
            times.append(1e3 * t0.elapsed_time(t1) / a.frames)
            s.close()
        print(f"{name}: {a.slots} slots, {a.frames} frames: " + ", ".join(f"{t:.1f}" for t in times) + " us per frame (events)", flush=True)


if __name__ == "__main__":
    main()
