"""Objects created on a busy non-blocking stream (a serving thread's frame stream with ticks queued): their slab's zero fill is
queued on that stream, while the C create call initialises the slab at once (plain hipMemcpy / hipMemset / a null-stream kernel).
The fill must not land on top of that initialisation.  The scheduler creates its stream resampler and codec sessions this way,
on the first request that needs them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _busy(stream):
    with torch.cuda.stream(stream):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(24):
            x = torch.tanh(x @ x)
    return x


def _convert(rs, pcm):
    rs.reset_slots([0], ["pcm_16000"])
    out, counts = rs.new_outputs(1)
    rs.chunk(pcm, pcm.shape[1], out, counts)
    return out, counts


def test_resampler_created_on_a_busy_stream_converts_like_one_created_idle():
    from smoltts_amd.codec.synthetic import synthetic_pcm
    from smoltts_amd.engine import Resampler

    dev = torch.device("cuda", torch.cuda.current_device())
    pcm = torch.from_numpy(np.asarray(synthetic_pcm(2 * 1920, 4), np.float32) * 0.5)[None].to(dev).contiguous()
    ref = Resampler(dev, 1, 2 * 1920)
    want = [t.cpu().numpy() for t in _convert(ref, pcm)]
    torch.cuda.synchronize()
    busy = torch.cuda.Stream()
    keep = _busy(busy)
    with torch.cuda.stream(busy):
        rs = Resampler(dev, 1, 2 * 1920)  # created behind tens of milliseconds of queued work
        got = _convert(rs, pcm)
    busy.synchronize()
    got = [t.cpu().numpy() for t in got]
    del keep
    assert np.array_equal(got[1], want[1]) and int(want[1][0, 0]) > 0
    n = 2 * int(want[1][0, 0])
    assert np.array_equal(got[0][0, :n], want[0][0, :n]), "the resampler's tables were overwritten by its slab's zero fill"
    assert np.any(want[0][0, :n] != 0)
