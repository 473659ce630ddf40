"""Time the watermark stage (csrc/watermark.hip) at serving shape: 32 slots, 4 frames (7680 samples) per pass, or ``--wide``: a row
as wide as one behind the seam.  Prints the mean time per pass from device events; run it under
``rocprofv3 --kernel-trace --stats -- python3 tools/time_watermark.py`` for the kernel's own time."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import Watermarker  # noqa: E402
from smoltts_amd.watermark import Watermark  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--wide", action="store_true", help="rows of frames * 1920 + 24240 samples (behind the seam)")
    ap.add_argument("--passes", type=int, default=200)
    a = ap.parse_args()
    n_in = a.frames * 1920 + (24240 if a.wide else 0)
    x = torch.randn(a.slots, n_in, device="cuda") * 0.1
    wm = Watermark(0x0123456789ABCDEF)
    st = Watermarker(x.device, a.slots, wm)
    st.reset_slots(list(range(a.slots)), [wm.gain] * a.slots)
    out, counts = st.new_outputs(a.slots, n_in)
    for _ in range(20):
        st.chunk(x, n_in, out, counts)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.passes):
        st.chunk(x, n_in, out, counts)
    t1.record()
    torch.cuda.synchronize()
    print(f"{a.slots} slots x {n_in} samples: {1e3 * t0.elapsed_time(t1) / a.passes:.2f} us per pass (events, back to back)")
    st.close()


if __name__ == "__main__":
    main()
