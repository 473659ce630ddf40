"""Time the stream-format conversion (csrc/resample.hip) at serving shape: 32 slots, 4 frames (7680 samples) per pass, the six
formats spread over the slots.  Prints the mean time per pass from device events; run it under
``rocprofv3 --kernel-trace --stats -- python3 tools/time_resample.py`` for the kernel's own time."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import Resampler  # noqa: E402
from smoltts_amd.formats import STREAM_FORMATS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--passes", type=int, default=200)
    a = ap.parse_args()
    n_in = a.frames * 1920
    x = torch.randn(a.slots, n_in, device="cuda") * 0.3
    rs = Resampler(x.device, a.slots, n_in)
    rs.reset_slots(list(range(a.slots)), [STREAM_FORMATS[b % len(STREAM_FORMATS)] for b in range(a.slots)])
    out, counts = rs.new_outputs(a.slots)
    for _ in range(20):
        rs.chunk(x, n_in, out, counts)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.passes):
        rs.chunk(x, n_in, out, counts)
    t1.record()
    torch.cuda.synchronize()
    print(f"{a.slots} slots x {n_in} samples: {1e3 * t0.elapsed_time(t1) / a.passes:.2f} us per pass (events, back to back)")
    rs.close()


if __name__ == "__main__":
    main()
