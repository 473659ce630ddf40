"""``StreamConverter`` on the device against its own stages driven by hand: four slots (one with every option, segmented; a plain
one; a stretched and limited float32 one that is restarted as a FLAC stream; a loudness and ulaw_8000 one) over eight calls with
a short row, an end and a restart.  The converter's loop is what is held here: routing, through copies, control passing and
host reads.  Each stage's own bits are held to its numpy model by its own suite."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import engine, watermark as W  # noqa: E402
from smoltts_amd.flac import stream_header  # noqa: E402
from smoltts_amd.formats import ENC_ULAW  # noqa: E402
from smoltts_amd.request import parse_request  # noqa: E402
from smoltts_amd.tsm import out_bound  # noqa: E402

from limiter_helpers import driven  # noqa: E402

B, N_IN, CALLS = 4, 1920, 8
KEY = W.Watermark(0x0123456789ABCDEF, -26.0)
REQUESTS = [dict(trim_silence=True, loudness=-20.0, speed=1.25, watermark=True, peak_limit_db=-6.0, output_format="pcm_16000",
                 container="flac"),
            dict(),
            dict(speed=1.25, peak_limit_db=-6.0),
            dict(loudness=-16.0, output_format="ulaw_8000")]
MARKED = [True, False, False, False]
SEGMENT = (480, engine.SEAM_FIRST | engine.SEAM_FINAL, 240)  # slot 0's only segment: its pause, flags and lead
RESTART_BEHIND, RESTARTED = 4, dict(container="flac")  # slot 2's next tenant, started behind call 4: FLAC of the float32
SHORT = (2, 3, 1000)  # (call, slot, valid samples): one row with fewer real samples than the call is wide


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _calls(device):
    """(pcm, valid, last, seg_end, whether the call is the final one) of each call: noise-like speech driven +12 dB, so that
    every limited slot limits."""
    x = np.stack([driven(60 + b, 12.0)[:CALLS * N_IN] for b in range(B)])
    for f in range(CALLS):
        valid = np.full(B, N_IN, np.int32)
        if f == SHORT[0]:
            valid[SHORT[1]] = SHORT[2]
        end = np.full(B, int(f == CALLS - 1), np.int32)
        yield (torch.from_numpy(x[:, f * N_IN:(f + 1) * N_IN].copy()).to(device), torch.from_numpy(valid).to(device),
               torch.from_numpy(end).to(device), torch.from_numpy(end.copy()).to(device), f == CALLS - 1)


def run_converter(device):
    """Each slot's chunks (bytes) from the converter, started from the parsed requests."""
    opts = [parse_request("x", stream=True, **kw) for kw in REQUESTS]
    conv = engine.StreamConverter(device, B, N_IN, watermark=KEY)
    try:
        conv.start(list(range(B)), opts, MARKED)
        conv.start_segments([0], [SEGMENT[0]], [SEGMENT[1]], [SEGMENT[2]])
        assert conv.ends(range(B)) == (True, True)
        got = [[] for _ in range(B)]
        for f, (pcm, valid, last, seg_end, final) in enumerate(_calls(device)):
            p = conv.run(pcm, N_IN, valid, last, seg_end=seg_end)
            p.to_host(torch.cuda.current_stream())
            torch.cuda.synchronize()
            for b in range(B):
                assert p.converts(b) == (b != 1)
                if p.converts(b):
                    got[b].append(p.chunk(b, final).tobytes())
            if f == RESTART_BEHIND:
                conv.start([2], [parse_request("x", stream=True, **RESTARTED)], [False])
                assert conv.ends(range(B)) == (True, True)
        return got
    finally:
        conv.close()


def run_by_hand(device):
    """The same chunks from the eight stages driven one by one, in the order and with the through copies that
    ``StreamConverter.run`` had when every stage stood in it by name."""
    o0, o1, o2, o3 = [parse_request("x", stream=True, **kw) for kw in REQUESTS]
    every, OFF = list(range(B)), engine.SEAM_OFF
    tr, sj, ln, ts = (cls(device, B) for cls in (engine.SilenceTrimmer, engine.SeamJoiner, engine.LoudnessNormalizer, engine.TimeStretcher))
    wm, lim, fl = engine.Watermarker(device, B, KEY), engine.PeakLimiter(device, B), engine.FlacEncoder(device, B)
    rs = engine.Resampler(device, B, out_bound(N_IN))
    stages = (tr, sj, ln, ts, wm, lim, rs, fl)
    try:
        tr.start_segments(every, [engine.SEAM_FIRST | engine.SEAM_FINAL, OFF, OFF, OFF], [True, False, False, False], [0] * B,
                          [o.silence_thr for o in (o0, o1, o2, o3)])
        ln.reset_slots(every, [-20.0, None, None, -16.0], [0.0] * B)
        ts.reset_slots(every, [o0.speed_q, 65536, o2.speed_q, 65536])
        wm.reset_slots(every, [KEY.gain, 0.0, 0.0, 0.0])
        lim.reset_slots(every, [o0.ceiling, 0.0, o2.ceiling, 0.0])
        rs.reset_slots(every, ["pcm_16000", "pcm_24000", "pcm_24000", "ulaw_8000"])
        fl.reset_slots(every, [16000, 24000, 24000, 8000], [engine.FLAC_S16, engine.FLAC_OFF, engine.FLAC_OFF, engine.FLAC_OFF])
        tr.start_segments([0], [SEGMENT[1]], [True], [0], [o0.silence_thr])
        sj.start_segments([0], [SEGMENT[0]], [SEGMENT[1]], [SEGMENT[2]])

        def through(served, plain, out, counts, pcm, n_in, valid):
            """The rows of the slots a float stage does not serve, that a later stage does, take what it read."""
            if not plain:
                return counts
            mask = torch.zeros(B, dtype=torch.int32, device=device)
            mask[served] = 1
            out[plain, :n_in] = pcm[plain]
            return torch.where(mask != 0, counts, valid)

        got, owed, restarted = [[] for _ in range(B)], {0: 16000}, False
        for f, (pcm, valid, last, seg_end, final) in enumerate(_calls(device)):
            n_in = N_IN
            # slot 2 goes through the stretch and the limiter until it is restarted, then through FLAC alone
            two, not_two = ([], [2]) if restarted else ([2], [])
            out, counts = tr.new_outputs(B, n_in)
            tr.chunk(pcm, n_in, out, counts, valid=valid, seg_end=seg_end, last=last)
            valid, pcm, n_in = through([0], [2, 3], out, counts, pcm, n_in, valid), out, out.shape[1]
            out, counts = sj.new_outputs(B, n_in)
            sj.chunk(pcm, n_in, out, counts, valid=valid, seg_end=seg_end, last=last)
            valid, pcm, n_in = through([0], [2, 3], out, counts, pcm, n_in, valid), out, out.shape[1]
            out, counts = ln.new_outputs(B, n_in)
            ln.chunk(pcm, n_in, out, counts, valid=valid)
            valid, pcm, n_in = through([0, 3], [2], out, counts, pcm, n_in, valid), out, out.shape[1]
            out, counts = ts.new_outputs(B, n_in)
            ts.chunk(pcm, n_in, out, counts, valid=valid, last=last)
            valid, pcm, n_in = through([0] + two, not_two + [3], out, counts, pcm, n_in, valid), out, out.shape[1]
            out, counts = wm.new_outputs(B, n_in)
            wm.chunk(pcm, n_in, out, counts, valid=valid)
            valid, pcm, n_in = through([0], [2, 3], out, counts, pcm, n_in, valid), out, out.shape[1]
            out, counts = lim.new_outputs(B, n_in)
            lim.run(pcm, n_in, out, counts, valid, last)
            valid, pcm, n_in = through([0] + two, not_two + [3], out, counts, pcm, n_in, valid), out, out.shape[1]
            lim_out, lim_counts = out, counts
            s16, s16_counts = rs.new_outputs(B, n_in)
            rs.chunk(pcm, n_in, s16, s16_counts, valid=valid)
            frames, sizes = fl.new_outputs(B, max(n_in, s16.shape[1] // 2))  # (slot 0 is framed from the resampler's int16)
            fl.chunk(B, frames, sizes, pcm=pcm, n_in=n_in, valid=valid, s16=s16, s16_counts=s16_counts, last=last)
            torch.cuda.synchronize()
            lim_out, lim_counts, s16, s16_counts, frames, sizes = (t.cpu().numpy() for t in (lim_out, lim_counts, s16, s16_counts, frames, sizes))
            for b in [0] + not_two:
                data = b"".join(engine.FlacEncoder.slot_frames(frames, sizes, b))
                got[b].append((stream_header(owed.pop(b)) if b in owed else b"") + data)  # the header once per stream
            if two:
                got[2].append(lim_out[2, :int(lim_counts[2])].tobytes())
            got[3].append(rs.slot_bytes(s16, s16_counts, 3, tail=final, enc=ENC_ULAW).tobytes())
            if f == RESTART_BEHIND:
                tr.start_segments([2], [OFF], [False], [0], [o2.silence_thr])
                ln.reset_slots([2], [None], [0.0])
                ts.reset_slots([2], [65536])
                wm.reset_slots([2], [0.0])
                lim.reset_slots([2], [0.0])
                rs.reset_slots([2], ["pcm_24000"])
                fl.reset_slots([2], [24000], [engine.FLAC_F32])
                sj.start_segments([2], [0], [OFF])
                restarted, owed[2] = True, 24000
        return got
    finally:
        for st in stages:
            st.close()


def test_the_converter_equals_its_stages_driven_by_hand(device):
    got, want = run_converter(device), run_by_hand(device)
    assert got[1] == [] and want[1] == []  # the plain slot converts nothing
    for b in (0, 2, 3):
        assert len(got[b]) == len(want[b]) == CALLS
        for f in range(CALLS):
            assert got[b][f] == want[b][f], (b, f, len(got[b][f]), len(want[b][f]))
    assert all(sum(map(len, got[b])) > 1000 for b in (0, 2, 3))
    assert got[0][0].startswith(stream_header(16000)) and got[2][RESTART_BEHIND + 1].startswith(stream_header(24000))
