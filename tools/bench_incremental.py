"""Latency of text fed in pieces, in the setup of tools/bench_scheduler.py: smoltts_byte_150m synthetic weights,
32 slots, greedy, a background of plain streams that keeps about three quarters of the slots speaking.

    python tools/bench_incremental.py [trials] [frames_per_tick]

Per trial, three figures:
  plain   submit(sentence 1, stream=True) to its first chunk -- the reference for the next figure
  first   the feed that settles sentence 1 of an incremental request to its first chunk
  seam    sentence 2 is fed while segment 1 speaks; the time from segment 1's last chunk to segment 2's first, less the seam's
          pause being spoken (the chunks carry it), against the median time between two chunks inside segment 1: the extra gap
          the change of segment costs"""
import sys
import threading
import time

import numpy as np

sys.path.insert(0, ".")
from smoltts_amd import SmolTTS  # noqa: E402
from smoltts_amd.codec.synthetic import synthetic_mimi_state  # noqa: E402
from smoltts_amd.config import GenerationSettings  # noqa: E402
from smoltts_amd.server.scheduler import BatchScheduler  # noqa: E402
from smoltts_amd.synthetic import named_config, synthetic_lm_state  # noqa: E402

S1, S2 = "The first sentence is here.", "Another one follows it, and it is the last one."
FRAMES = 96  # per segment (the synthetic model never stops by itself)


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    tick = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    cfg = named_config("smoltts_byte_150m")
    tts = SmolTTS(state=synthetic_lm_state(cfg, seed=0), config=cfg, mimi_state=synthetic_mimi_state(seed=0))
    sched = BatchScheduler(tts, max_batch=32, frames_per_tick=tick, generation_settings=GenerationSettings.greedy(max_new_tokens=400))
    opts = {"max_bytes": 32, "pause_s": 0.25}
    list(sched.iter_chunks(sched.submit("warm up the stream path", "heart", stream=True, max_new_tokens=8)))
    list(sched.iter_chunks(sched.submit(f"{S1} {S2}", "heart", stream=True, max_new_tokens=8, segment=opts)))
    stop = threading.Event()

    def background(i):
        rng = np.random.default_rng(i)
        while not stop.is_set():
            for _ in sched.iter_chunks(sched.submit("background speech " * 3, "heart", stream=True, max_new_tokens=int(rng.integers(64, 385)))):
                pass

    threads = [threading.Thread(target=background, args=(i,), daemon=True) for i in range(24)]
    for t in threads:
        t.start()
    time.sleep(1.0)
    plain, first, seam_gap, step = [], [], [], []
    for _ in range(trials):
        t0 = time.perf_counter()
        it = sched.iter_chunks(sched.submit(S1, "heart", stream=True, max_new_tokens=FRAMES - 1))
        next(it)
        plain.append((time.perf_counter() - t0) * 1e3)
        for _c in it:
            pass
        r = sched.submit_incremental("heart", max_new_tokens=FRAMES - 1, segment=opts)
        r.feed(S1)
        t0 = time.perf_counter()
        r.feed(" Another")  # sentence 1 is settled: "Another" cannot be packed beside it
        times, sizes = [], []
        for j, c in enumerate(r):
            times.append(time.perf_counter())
            sizes.append(c.shape[0])
            if j == 0:
                first.append((times[0] - t0) * 1e3)
                r.feed(S2[len("Another"):])
                r.close()  # segment 2 is known, and known to be the last, long before segment 1 ends
        done = np.cumsum(sizes)
        seg1 = FRAMES * 1920 + 6000  # segment 1's samples and the seam's pause (the synthetic codec is never silent)
        k = int(np.searchsorted(done, seg1, side="right"))  # the first chunk with samples of segment 2
        if 0 < k < len(times):
            seam_gap.append((times[k] - times[k - 1]) * 1e3)
            step.append(float(np.median(np.diff(times[1:k]))) * 1e3)
    stop.set()
    q = lambda v: f"p50 {np.median(v):.2f} ms, max {np.max(v):.2f} ms" if v else "none"
    print(f"{trials} trials, tick {tick}, 24 background streams in 32 slots")
    print(f"  plain stream of sentence 1, submit to first chunk:        {q(plain)}")
    print(f"  incremental, settling feed of sentence 1 to first chunk:  {q(first)}")
    print(f"  segment 1's last chunk to segment 2's first:              {q(seam_gap)}  (between two chunks inside segment 1: {q(step)})")
    for t in threads:
        t.join(timeout=60)
    sched.close()


if __name__ == "__main__":
    main()
