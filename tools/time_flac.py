"""Time the FLAC framing of streams (csrc/flac.hip) at serving shape: 32 slots, one 4-frame pass each (7680 codec samples), half at
24 kHz from fp32 and half at 48 kHz from the resampler's int16; ``--speed 0.5`` stretches every other slot first.  Prints the mean
time per pass from device events (the whole StreamConverter pass, and the FLAC launch alone); run it under
``rocprofv3 --kernel-trace --stats -- python3 tools/time_flac.py`` for the kernels' own times."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import FLAC_F32, FLAC_S16, FlacEncoder, StreamConverter  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--speed", type=float, default=None, help="stretch every other slot at this speed (e.g. 0.5)")
    a = ap.parse_args()
    n_in = a.frames * 1920
    B = a.slots
    x = torch.randn(B, n_in, device="cuda") * 0.3
    valid = torch.full((B,), n_in, dtype=torch.int32, device="cuda")
    last = torch.zeros(B, dtype=torch.int32, device="cuda")
    conv = StreamConverter(x.device, B, n_in)
    sq = [None if a.speed is None or b % 2 else int(round(a.speed * 65536)) for b in range(B)]
    conv.reset_slots(list(range(B)), ["pcm_24000" if b % 2 == 0 else "pcm_48000" for b in range(B)], sq, ["flac"] * B)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        conv.run(x, n_in, valid, last)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(a.passes):
        conv.run(x, n_in, valid, last)
    t1.record()
    torch.cuda.synchronize()
    whole = t0.elapsed_time(t1) * 1e3 / a.passes
    # the FLAC launch alone, on the same shapes (fp32 rows of 7680 samples, int16 rows of 15360)
    fe = FlacEncoder(x.device, B)
    fe.reset_slots(list(range(B)), [24000 if b % 2 == 0 else 48000 for b in range(B)], [FLAC_F32 if b % 2 == 0 else FLAC_S16 for b in range(B)])
    s16 = (torch.randn(B, 2 * n_in, device="cuda") * 3000).to(torch.int16).view(torch.uint8).contiguous()
    counts = torch.tensor([[2 * n_in, 0]] * B, dtype=torch.int32, device="cuda")
    out, sizes = fe.new_outputs(B, 2 * n_in)
    for _ in range(20):
        fe.chunk(B, out, sizes, pcm=x, n_in=n_in, valid=valid, s16=s16, s16_counts=counts, last=last)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(a.passes):
        fe.chunk(B, out, sizes, pcm=x, n_in=n_in, valid=valid, s16=s16, s16_counts=counts, last=last)
    t1.record()
    torch.cuda.synchronize()
    alone = t0.elapsed_time(t1) * 1e3 / a.passes
    print(f"{B} slots x {n_in} samples, speed {a.speed}: StreamConverter pass {whole:.1f} us, FLAC launch {alone:.1f} us")
    fe.close()
    conv.close()


if __name__ == "__main__":
    main()
