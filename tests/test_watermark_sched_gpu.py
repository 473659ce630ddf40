"""The watermark through the front ends on the tiny checkpoint: ``SmolTTS`` (blocking, streamed, segmented), ``BatchScheduler``
(blocking, streamed, stretched, converted, segmented; unmarked requests before and after the stage exists) and the HTTP routes
behind a scheduler.  Marked audio equals the numpy model over the unmarked run's audio, and is detected."""
import base64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import watermark as W  # noqa: E402

KEY = W.Watermark(0x0123456789ABCDEF, -26.0)
TEXT = 'The first sentence is here. A second one follows it! <break time="0.5s"/> And then a third, which ends the text.'
OPTS = {"max_bytes": 40, "pause_s": 0.2}
SHORT = "Mark this sentence, please."
FRAMES = 30  # 2.4 s of audio per utterance: the detector's 2 s case


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _models():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = named_config("tiny")
    kw = dict(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))
    return SmolTTS(**kw), SmolTTS(**kw, watermark=KEY)


@pytest.fixture(scope="module")
def models():
    return _models()


def _detected(pcm, rate=24000, offset=0):
    d = W.detect(pcm, KEY.key, rate)
    print(f"{np.asarray(pcm).size} samples at {rate} Hz: score {d.score:.2f} at offset {d.offset}")
    return d.detected and (offset is None or d.offset == offset)


def test_facade_blocking_stream_and_segmented(models):
    from smoltts_amd.config import GenerationSettings

    tts, tts_w = models
    gs = GenerationSettings.greedy(max_new_tokens=FRAMES)
    plain = tts(SHORT, "nova", generation_settings=gs)
    assert plain.size >= 48000, "the tiny checkpoint must speak 2 s for the detection below to say anything"
    got = tts_w(SHORT, "nova", generation_settings=gs)
    assert np.array_equal(_bits(got), _bits(W.embed(plain, KEY))) and _detected(got) and not _detected(plain)
    assert np.array_equal(_bits(tts_w(SHORT, "nova", generation_settings=gs, watermark=False)), _bits(plain))  # asked off: today's bytes
    with pytest.raises(ValueError, match="watermark"):
        tts(SHORT, "nova", generation_settings=gs, watermark=True)  # no key
    with pytest.raises(ValueError, match="watermark"):
        tts_w(SHORT, "nova", generation_settings=gs, watermark=1)
    # behind the stretch: the chips keep their rate
    fast = tts(SHORT, "nova", generation_settings=gs, speed=1.25)
    assert np.array_equal(_bits(tts_w(SHORT, "nova", generation_settings=gs, speed=1.25)), _bits(W.embed(fast, KEY)))
    # streams: frame by frame, the bytes of the whole
    ref = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs)))
    chunks = list(tts_w.stream(SHORT, "nova", generation_settings=gs))
    assert all(c.size == 1920 for c in chunks)  # every frame's samples leave with the frame
    assert np.array_equal(_bits(np.concatenate(chunks)), _bits(W.embed(ref, KEY))) and _detected(np.concatenate(chunks))
    s16 = np.concatenate(list(tts_w.stream(SHORT, "nova", generation_settings=gs, output_format="pcm_16000")))
    assert s16.dtype == np.int16 and _detected(s16, 16000)
    # a segmented stream keeps one mark grid across its seams: the model over the joined audio, from position 0
    ref = np.concatenate(list(tts.stream(TEXT, "sky", generation_settings=gs, segment=OPTS)))
    got = np.concatenate(list(tts_w.stream(TEXT, "sky", generation_settings=gs, segment=OPTS)))
    assert len(tts_w.last_segments) >= 3
    assert np.array_equal(_bits(got), _bits(W.embed(ref, KEY))) and _detected(got, offset=0)


def test_scheduler_and_http(models):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    tts, _ = models
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=FRAMES),
                           watermark=KEY)
    try:
        def run(text=SHORT, voice="nova", **kw):
            req = sched.submit(text, voice, **kw)
            return np.concatenate(list(sched.iter_chunks(req))), req

        # asked off, before any request has been marked: the routes as they were, and no stage
        (plain, r0), (raw0, _), (fast0, _) = run(watermark=False), run(stream=True, watermark=False), run(speed=1.25, watermark=False)
        (seg0, _) = run(TEXT, "sky", stream=True, segment=OPTS, watermark=False)
        assert sched._stream_conv.wm is None and r0.watermark is False and plain.size >= 48000
        # the scheduler's policy: a request that does not say is marked
        block, r1 = run()
        assert r1.watermark is True and np.array_equal(_bits(block), _bits(W.embed(plain, KEY))) and _detected(block)
        assert sched._stream_conv.wm is None  # (a blocking request is marked whole, outside the stream converter)
        stream, _ = run(stream=True)
        assert sched._stream_conv.wm is not None
        assert np.array_equal(_bits(stream), _bits(W.embed(raw0, KEY))) and _detected(stream)
        fast, _ = run(speed=1.25)
        assert np.array_equal(_bits(fast), _bits(W.embed(fast0, KEY)))
        seg, _ = run(TEXT, "sky", stream=True, segment=OPTS)
        assert np.array_equal(_bits(seg), _bits(W.embed(seg0, KEY))) and _detected(seg, offset=0)  # one grid across the seams
        # asked off again, now that the stage exists, alone and beside marked streams: the same bytes as before
        assert np.array_equal(_bits(run(stream=True, watermark=False)[0]), _bits(raw0))
        assert np.array_equal(_bits(run(watermark=False)[0]), _bits(plain))
        reqs = [sched.submit(SHORT, "nova", stream=True), sched.submit(SHORT, "nova", stream=True, watermark=False),
                sched.submit(SHORT, "nova", stream=True, output_format="pcm_16000")]
        a, b, c16 = [np.concatenate(list(sched.iter_chunks(r))) for r in reqs]
        assert np.array_equal(_bits(b), _bits(raw0)) and np.array_equal(_bits(a), _bits(W.embed(raw0, KEY)))
        assert c16.dtype == np.int16 and _detected(c16, 16000)
        with pytest.raises(ValueError, match="watermark"):
            sched.submit(SHORT, "nova", watermark="yes")

        setting = {"key": "0123456789abcdef", "strength_db": -26.0, "apply": "cloned"}
        c = TestClient(create_app(tts, settings={"watermark": setting}, scheduler=sched))
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova"})
        assert r.status_code == 200 and "x-watermark" not in r.headers and r.content == pcm_to_wav_bytes(plain, 24000)  # a preset voice
        c = TestClient(create_app(tts, settings={"watermark": dict(setting, apply="all")}, scheduler=sched))
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova"})
        assert r.status_code == 200 and r.headers["x-watermark"] == "1" and r.content == pcm_to_wav_bytes(W.embed(plain, KEY), 24000)
        d = c.post("/v1/watermark/detect", json={"audio": base64.b64encode(r.content).decode()})
        assert d.status_code == 200 and d.json()["detected"] is True
        r = c.post("/v1/text-to-speech/nova/stream?output_format=ulaw_8000", json={"text": SHORT})
        assert r.status_code == 200 and r.headers["x-watermark"] == "1" and len(r.content) > 8000
    finally:
        sched.close()
