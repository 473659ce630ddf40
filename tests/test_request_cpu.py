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


# ------------------------------------------------------------------------------- the value rebuilds its own keywords
SEG5 = SegmentOptions(max_bytes=5, pause_s=0.25, context="previous")
# (text, stream, the caller's keywords, what ``GpuPool.submit`` hands its worker for them: recorded from the pool before
# ``SpeechOptions.given`` existed, when it built the dict by hand)
TABLE = [
    ("Hello.", False, {}, {}),
    ("Hello.", False, dict(speed=1.0), {}),
    ("Hello.", False, dict(speed=1.5, loudness=-20), {"speed": 1.5, "loudness": -20.0}),
    ("Hello.", True, dict(output_format="pcm_24000"), {}),
    ("Hello.", True, dict(output_format="pcm_16000", container="flac"), {"output_format": "pcm_16000", "container": "flac"}),
    ("Hello.", True, dict(loudness=-18.0), {"loudness": -18.0}),
    ("Hello.", True, dict(loudness=-18.0, loudness_start_gain_db=-3.0), {"loudness": -18.0, "loudness_start_gain_db": -3.0}),
    ("Hello.", False, dict(max_pause_s=0.5), {"max_pause_s": 0.5}),
    ("Hello.", False, dict(trim_silence=True, silence_threshold_db=-40.0), {"trim_silence": True, "silence_threshold_db": -40.0}),
    ("One. Two.", False, dict(segment=True), {"segment": SegmentOptions(max_bytes=300, pause_s=0.25, context="previous")}),
    ("One. Two.", True, dict(segment={"max_bytes": 5}), {"segment": SEG5}),
    ("Hello.", False, dict(peak_limit_db=0.0), {"peak_limit_db": 0.0}),
    ("Hello.", False, dict(timestamps=True), {"timestamps": True}),
    ("Hello.", True, dict(watermark=True), {"watermark": True}),
    ("Hello.", False, dict(watermark=False, trim_silence=False), {"watermark": False}),
    ("One. Two.", True, dict(output_format="ulaw_8000", speed=0.8, loudness=-23.0, loudness_start_gain_db=2.5, trim_silence=True,
                              max_pause_s=0.25, silence_threshold_db=-50.0, peak_limit_db=-6.0, watermark=False,
                              segment={"max_bytes": 5, "pause_s": 0.1}),
     {"output_format": "ulaw_8000", "speed": 0.8, "segment": SegmentOptions(max_bytes=5, pause_s=0.1, context="previous"),
      "loudness": -23.0, "loudness_start_gain_db": 2.5, "watermark": False, "trim_silence": True, "max_pause_s": 0.25,
      "silence_threshold_db": -50.0, "peak_limit_db": -6.0}),
]
OPTION_NAMES = {"output_format", "speed", "container", "segment", "loudness", "loudness_start_gain_db", "watermark", "trim_silence",
                "max_pause_s", "silence_threshold_db", "timestamps", "peak_limit_db"}


def _same(a, b):
    """Two parsed values are equal, their plans compared by their segments."""
    import dataclasses

    segs = lambda p: None if p.plan is None else p.plan.segs  # noqa: E731
    return dataclasses.replace(a, plan=None) == dataclasses.replace(b, plan=None) and segs(a) == segs(b)


def test_the_table_turns_every_option_on():
    import inspect

    assert len(TABLE) >= 12 and {k for _, _, kw, _ in TABLE for k in kw} == OPTION_NAMES
    assert OPTION_NAMES == set(inspect.signature(parse_request).parameters) - {"text", "stream", "pieces"}


@pytest.mark.parametrize("text,stream,kw,sent", TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_given_round_trips(text, stream, kw, sent):
    p = parse_request(text, stream=stream, **kw)
    assert p.given() == sent  # (the keys and values the pool has always sent: see below)
    assert _same(parse_request(text, stream=stream, **p.given()), p)
    assert parse_request(text, stream=stream).given() == {} and parse_request().given() == {}


def _pool():
    """A pool without workers whose one worker queue is a list."""
    import itertools
    import threading

    from smoltts_amd.server.pool import GpuPool

    class Alive:
        def is_alive(self):
            return True

    class Queue(list):
        put = list.append

    pool = GpuPool.__new__(GpuPool)
    pool._lock, pool._closing, pool._dead, pool._load, pool._reqs, pool._ids = threading.Lock(), False, [False], [0], {}, itertools.count(1)
    pool._procs, pool._req_qs = [Alive()], [Queue()]
    pool._settings, pool.watermark, pool.alignment_heads = None, object(), [(0, 0)]
    return pool


@pytest.mark.parametrize("text,stream,kw,sent", TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_the_pool_sends_its_worker_the_keys_it_always_sent(text, stream, kw, sent):
    from smoltts_amd.server.pool import GpuPool

    pool = _pool()
    GpuPool.submit(pool, text, stream=stream, **kw)
    (msg,) = pool._req_qs[0]
    assert msg == ("submit", 1, text, "heart", stream, None) + ((sent,) if sent else ())


def test_an_unknown_option_is_a_type_error_in_every_front_end_before_any_work():
    from smoltts_amd import SmolTTS
    from smoltts_amd.server.pool import GpuPool
    from smoltts_amd.server.scheduler import BatchScheduler

    with pytest.raises(TypeError, match="peak_limit"):
        parse_request("x", peak_limit=-3.0)
    for front, call in ((GpuPool, GpuPool.submit), (BatchScheduler, BatchScheduler.submit), (SmolTTS, SmolTTS.__call__)):
        with pytest.raises(TypeError, match="peak_limit"):
            call(front.__new__(front), "x", peak_limit=-3.0)
    for front, call in ((GpuPool, GpuPool.submit_incremental), (BatchScheduler, BatchScheduler.submit_incremental)):
        with pytest.raises(TypeError, match="loudnes"):
            call(front.__new__(front), "nova", loudnes=-20.0)
    with pytest.raises(TypeError, match="peak_limit"):
        next(SmolTTS.stream(SmolTTS.__new__(SmolTTS), "x", peak_limit=-3.0))
    with pytest.raises(TypeError, match="peak_limit"):
        next(SmolTTS.stream(SmolTTS.__new__(SmolTTS), iter(["x"]), peak_limit=-3.0))
    with pytest.raises(ValueError, match="output_format applies to streaming requests"):
        SmolTTS.__call__(SmolTTS.__new__(SmolTTS), "x", output_format="pcm_16000")
