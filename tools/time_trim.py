"""Time the trim stage (csrc/trim.hip) beside the seam stage (csrc/seam.hip) at serving shape: 32 slots, 4 frames (7680 samples)
per pass.  Three signals: speech (no block is silent: every block is judged and copied out), a pause (every block is silent and
the slots hold all they can: the held blocks move from one state half to the other every pass), and a pause of 8 passes followed
by speech, over and over (the hold fills and is released).  Prints the mean time per pass from device events, the two stages
alternating in rounds."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smoltts_amd.engine import SEAM_FIRST, SeamJoiner, SilenceTrimmer  # noqa: E402
from smoltts_amd.seam import THRESH  # noqa: E402


def timed(call, passes):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(passes):
        call()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--passes", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    B, n_in = a.slots, a.frames * 1920
    dev = torch.device("cuda", 0)
    speech = torch.randn(B, n_in, device=dev) * 0.1
    quiet = torch.randn(B, n_in, device=dev) * 1e-4
    slots = list(range(B))
    tr, sj = SilenceTrimmer(dev, B), SeamJoiner(dev, B)
    t_out, t_cnt = tr.new_outputs(B, n_in)
    s_out, s_cnt = sj.new_outputs(B, n_in)

    def open_slots(P):  # a first segment that is not the last: the seam holds trailing silence too; the trim holds for its tail
        tr.start_segments(slots, [3] * B, [1] * B, [P] * B, [float(THRESH)] * B)
        sj.start_segments(slots, [0] * B, [SEAM_FIRST] * B)

    cases = (("speech", [speech]), ("a pause, held", [quiet]), ("8 passes of a pause, then speech", [quiet] * 8 + [speech]))
    for name, seq in cases:
        for r in range(a.rounds):
            res = {}
            for stage in ("trim", "seam"):
                def cycle(stage=stage):
                    for x in seq:
                        if stage == "trim":
                            tr.chunk(x, n_in, t_out, t_cnt)
                        else:
                            sj.chunk(x, n_in, s_out, s_cnt)
                open_slots(0)
                if stage == "trim":  # (speech first: a pause that opens the stream is its head, of which 2 blocks are held)
                    tr.chunk(speech, n_in, t_out, t_cnt)
                else:
                    sj.chunk(speech, n_in, s_out, s_cnt)
                for _ in range(40):
                    cycle()
                torch.cuda.synchronize()
                res[stage] = timed(cycle, max(a.passes // len(seq), 1)) / len(seq)
            print(f"{B} slots x {n_in} samples, {name}, round {r}: trim {res['trim']:.2f} us, seam {res['seam']:.2f} us per pass", flush=True)
    tr.close()
    sj.close()


if __name__ == "__main__":
    main()
