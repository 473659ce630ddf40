"""Time the speaking-speed stretch (csrc/tsm.hip) at serving shape: 32 slots, 4 frames (7680 samples) per pass, every slot at
one speed.  Prints the mean time per pass from device events; run it under
``rocprofv3 --kernel-trace --stats -- python3 tools/time_tsm.py`` for the kernel's own time."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import TimeStretcher  # noqa: E402
from smoltts_amd.tsm import speed_q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--passes", type=int, default=100)
    ap.add_argument("--speeds", default="0.25,1.25,4")
    a = ap.parse_args()
    n_in = a.frames * 1920
    x = torch.randn(a.slots, n_in, device="cuda") * 0.3
    for s in (float(v) for v in a.speeds.split(",")):
        ts = TimeStretcher(x.device, a.slots)
        ts.reset_slots(list(range(a.slots)), [speed_q(s)] * a.slots)
        out, counts = ts.new_outputs(a.slots, n_in)
        for _ in range(10):
            ts.chunk(x, n_in, out, counts)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.passes):
            ts.chunk(x, n_in, out, counts)
        t1.record()
        torch.cuda.synchronize()
        print(f"speed {s}: {a.slots} slots x {n_in} samples -> {int(counts[0])} out: "
              f"{1e3 * t0.elapsed_time(t1) / a.passes:.2f} us per pass (events, back to back)")
        ts.close()


if __name__ == "__main__":
    main()
