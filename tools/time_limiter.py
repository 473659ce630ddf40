"""Time the limiter stage (csrc/limiter.hip) at serving shape: 32 slots, 4 frames (7680 samples) per pass, and 32 slots of 31920
samples (the in-launch rounds), every slot driven so that it limits.  The loudness and watermark stages run at the same shapes in
the same process as the yardstick.  Prints the mean time per pass from device events; run it under
``rocprofv3 --kernel-trace --stats -- python3 tools/time_limiter.py`` for the kernels' own times."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import LoudnessNormalizer, PeakLimiter, Watermarker  # noqa: E402
from smoltts_amd.limiter import ceiling_of_db  # noqa: E402
from smoltts_amd.watermark import Watermark  # noqa: E402


def timed(name, slots, n_in, passes, call):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(passes):
        call()
    t1.record()
    torch.cuda.synchronize()
    print(f"{name}: {slots} slots x {n_in} samples: {1e3 * t0.elapsed_time(t1) / passes:.2f} us per pass (events, back to back)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--widths", type=int, nargs="+", default=[7680, 31920])
    ap.add_argument("--ceiling-db", type=float, default=-12.0)
    ap.add_argument("--passes", type=int, default=200)
    a = ap.parse_args()
    slots = list(range(a.slots))
    dev = torch.device("cuda")
    lim = PeakLimiter(dev, a.slots)
    wm = Watermark(0x0123456789ABCDEF)
    mark = Watermarker(dev, a.slots, wm)
    loud = LoudnessNormalizer(dev, a.slots)
    for n_in in a.widths:
        x = torch.randn(a.slots, n_in, device=dev) * 0.5  # far over the ceiling: every window limits
        lim.reset_slots(slots, [ceiling_of_db(a.ceiling_db)] * a.slots)
        out, counts = lim.new_outputs(a.slots, n_in)
        timed("limiter", a.slots, n_in, a.passes, lambda: lim.chunk(x, n_in, out, counts))
        assert int(counts.min()) == n_in and float(out[:, :n_in].abs().max()) <= ceiling_of_db(a.ceiling_db) * (1 + 2.0 ** -23)
        assert lim.slot_state(0)["min_g"] < 1.0
        loud.reset_slots(slots, [-16.0] * a.slots)
        out, counts = loud.new_outputs(a.slots, n_in)
        timed("loudness", a.slots, n_in, a.passes, lambda: loud.chunk(x, n_in, out, counts))
        mark.reset_slots(slots, [wm.gain] * a.slots)
        out, counts = mark.new_outputs(a.slots, n_in)
        timed("watermark", a.slots, n_in, a.passes, lambda: mark.chunk(x, n_in, out, counts))
    for st in (lim, mark, loud):
        st.close()


if __name__ == "__main__":
    main()
