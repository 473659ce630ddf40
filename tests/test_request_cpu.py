"""The one parse of a speech request's options (smoltts_amd/request.py), and that every front end refuses what it refuses before
any work: the façade, the scheduler and the pool (no GPU: the refusals come before any state is touched)."""
import pytest

from smoltts_amd.formats import ENC_S16
from smoltts_amd.longform import SegmentOptions
from smoltts_amd.request import parse_request

BAD = [
    (dict(speed=0.1), r"\[0.25, 4.0\]"),
    (dict(stream=True, output_format="pcm_12345"), "unsupported stream output_format"),
    (dict(container="flac"), "container applies to streaming requests"),
    (dict(output_format="pcm_16000"), "output_format applies to streaming requests"),
    (dict(stream=True, container="flac", output_format="ulaw_8000"), "frames 16-bit PCM"),
    (dict(stream=True, container="ogg"), "unsupported container"),
    (dict(text='a <break time="9s"/> b', segment=True), "break time"),
    (dict(text=' <break time="1s"/> ', segment=True), "nothing to speak"),
    (dict(segment="yes"), "segment must be"),
]


@pytest.mark.parametrize("kw,match", BAD)
def test_parse_refuses(kw, match):
    kw = dict(kw)
    with pytest.raises(ValueError, match=match):
        parse_request(kw.pop("text", "x"), **kw)


def test_parse_normalises():
    p = parse_request("Hello.")
    assert (p.output_format, p.speed, p.speed_q, p.container, p.segment, p.plan) == (None,) * 6
    p = parse_request("Hello.", stream=True, output_format="pcm_24000", speed=1.0, container="flac", segment=True)
    assert (p.output_format, p.speed, p.speed_q, p.container) == (None, None, None, "flac")
    assert p.segment == SegmentOptions() and p.plan is None  # one plain segment: the plain path
    p = parse_request("One. Two.", stream=True, output_format="pcm_16000", speed=1.5, segment={"max_bytes": 5})
    assert p.output_format == "pcm_16000" and p.speed == 1.5 and p.speed_q == round(65536 * 1.5)
    assert [s.text for s in p.plan.segs] == ["One.", "Two."]
    from smoltts_amd.formats import parse_stream_format

    assert parse_stream_format(p.output_format)[1] == ENC_S16


@pytest.mark.parametrize("kw,match", BAD)
def test_every_front_end_refuses_before_any_work(kw, match):
    from smoltts_amd import SmolTTS
    from smoltts_amd.server.pool import GpuPool
    from smoltts_amd.server.scheduler import BatchScheduler

    kw = dict(kw)
    text = kw.pop("text", "x")
    pool = GpuPool.__new__(GpuPool)  # (no workers: refused before any is chosen)
    with pytest.raises(ValueError, match=match):
        GpuPool.submit(pool, text, **kw)
    sched = BatchScheduler.__new__(BatchScheduler)  # (refused before the scheduler's state is touched)
    with pytest.raises(ValueError, match=match):
        BatchScheduler.submit(sched, text, **kw)
    tts = SmolTTS.__new__(SmolTTS)  # (refused before the model is touched)
    if kw.pop("stream", False):
        with pytest.raises(ValueError, match=match):
            next(SmolTTS.stream(tts, text, **kw))
    elif not {"output_format", "container"} & set(kw):  # (``__call__`` has neither)
        with pytest.raises(ValueError, match=match):
            SmolTTS.__call__(tts, text, **kw)
