"""Wall time of a ``best_of`` request against a plain one on an otherwise idle scheduler: ``--slots`` slots of the
``--model`` synthetic model, requests that run to ``--frames`` frames (the synthetic model never stops by itself), ``--runs`` runs
each, from ``submit`` to the last byte of audio."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd import SmolTTS  # noqa: E402
from smoltts_amd.codec.synthetic import synthetic_mimi_state  # noqa: E402
from smoltts_amd.config import GenerationSettings, RequestSampling  # noqa: E402
from smoltts_amd.server.scheduler import BatchScheduler  # noqa: E402
from smoltts_amd.synthetic import named_config, synthetic_lm_state  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="smoltts_byte_150m")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--best-of", type=int, default=4)
    a = ap.parse_args()
    cfg = named_config(a.model)
    tts = SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))
    sched = BatchScheduler(tts, max_batch=a.slots, generation_settings=GenerationSettings.greedy(max_new_tokens=a.frames))
    try:
        for name, n in (("warm-up", a.best_of), ("plain", 1), (f"best_of={a.best_of}", a.best_of), ("plain", 1), (f"best_of={a.best_of}", a.best_of)):
            times = []
            for k in range(a.runs):
                smp = RequestSampling(temperature=0.9, seed=100 + k, logprobs=True, best_of=n if n > 1 else None)
                t0 = time.perf_counter()
                size = sum(c.size for c in sched.iter_chunks(sched.submit("a request of a few words", "heart", sampling=smp)))
                times.append(1e3 * (time.perf_counter() - t0))
            print(f"{name}: {a.frames} frames, {size} samples: " + ", ".join(f"{t:.1f}" for t in times) + " ms from submit to the last byte", flush=True)
    finally:
        sched.close()


if __name__ == "__main__":
    main()
