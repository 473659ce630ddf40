"""The peak limiter through the front ends on the tiny checkpoint: ``SmolTTS`` (blocking and streamed), ``BatchScheduler`` (more
requests than slots, every other one limited), the HTTP routes behind a scheduler, and ``GpuPool``.  Limited audio equals the
numpy model (``limiter.py``) over the same call's audio without the option, bit for bit, and every case shows the limiter
engaged: a request at ``loudness=-5`` under ``peak_limit_db=-12`` cannot stay under its ceiling."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import limiter as LM, loudness  # noqa: E402

SHORT = "Limit this sentence, please."
FRAMES = 30  # 2.4 s: long enough for the loudness meter's blocks
LOUD, DB = -5.0, -12.0
STREAM_KW = dict(loudness=LOUD, loudness_start_gain_db=20.0)  # a stream that is loud from its first frame


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stream_model(ref, db):
    """``limiter.StreamState`` over the unlimited stream ``ref``, frame by frame; (its output, its smallest gain)."""
    st = LM.StreamState(db)
    out = [st.process(ref[i:i + 1920], last=i + 1920 >= ref.size) for i in range(0, ref.size, 1920)]
    return np.concatenate(out), float(st.min_g)


@pytest.fixture(scope="module")
def tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state=synthetic_mimi_state(seed=5))


@pytest.fixture(scope="module")
def gs():
    from smoltts_amd.config import GenerationSettings

    return GenerationSettings.greedy(max_new_tokens=FRAMES)


def test_facade_blocking_and_stream(tts, gs):
    plain = tts(SHORT, "nova", generation_settings=gs)
    assert plain.size >= 9600 and tts.last_peak_reduction_db is None
    # blocking: limited whole, last of all, behind the loudness gain, which is then not capped by the peak
    got = tts(SHORT, "nova", generation_settings=gs, loudness=LOUD, peak_limit_db=DB)
    level, g = loudness.normalize(plain, LOUD, cap=False)
    want, gmin = LM.limit(level, DB)
    print(f"blocking: loudness gain {loudness.gain_db(g):.2f} dB, peak {np.abs(level).max():.3f}, reduction {LM.reduction_db(gmin):.2f} dB")
    assert tts.last_peak_reduction_db == LM.reduction_db(gmin) > 0.0  # engaged
    assert tts.last_loudness_gain_db == loudness.gain_db(g) and g > loudness.normalize(plain, LOUD)[1]
    assert got.shape == plain.shape and np.array_equal(_bits(got), _bits(want))
    assert float(np.abs(got).max()) <= LM.ceiling_of_db(DB) * (1.0 + 2.0 ** -23)
    # behind the stretch as well
    fast = tts(SHORT, "nova", generation_settings=gs, loudness=LOUD, speed=1.25)
    capped_gain = tts.last_loudness_gain_db
    got = tts(SHORT, "nova", generation_settings=gs, loudness=LOUD, speed=1.25, peak_limit_db=DB)
    assert got.shape == fast.shape and tts.last_peak_reduction_db > 0.0 and tts.last_loudness_gain_db > capped_gain
    # a signal that stays under the ceiling returns the unlimited bytes
    quiet = tts(SHORT, "nova", generation_settings=gs, loudness=-40.0)
    assert float(np.abs(quiet).max()) < 1.0
    same = tts(SHORT, "nova", generation_settings=gs, loudness=-40.0, peak_limit_db=0.0)
    assert tts.last_peak_reduction_db == 0.0 and np.array_equal(_bits(same), _bits(quiet))
    with pytest.raises(ValueError, match="peak_limit_db"):
        tts(SHORT, "nova", generation_settings=gs, peak_limit_db=1.0)
    # the stream: the model over the unlimited stream, 126 samples late until the end
    ref = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, **STREAM_KW)))
    chunks = list(tts.stream(SHORT, "nova", generation_settings=gs, peak_limit_db=DB, **STREAM_KW))
    want, gmin = _stream_model(ref, DB)
    assert gmin < 1.0  # engaged
    assert chunks[0].size == 1920 - LM.HOLD_BACK and sum(c.size for c in chunks) == ref.size
    assert np.array_equal(_bits(np.concatenate(chunks)), _bits(want))
    assert np.array_equal(_bits(want), _bits(LM.limit(ref, DB)[0]))
    # ... in front of the conversion
    s16 = np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, peak_limit_db=DB, output_format="pcm_16000", **STREAM_KW)))
    assert s16.dtype == np.int16 and abs(s16.size - ref.size * 2 // 3) <= 1
    # a stream that never asks makes no stage: today's bytes
    assert np.array_equal(_bits(np.concatenate(list(tts.stream(SHORT, "nova", generation_settings=gs, **STREAM_KW)))), _bits(ref))


def test_scheduler_routes_and_pool(tts, gs):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler
    from smoltts_amd.server.scheduler import BatchScheduler
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    sched = BatchScheduler(tts, max_batch=2, frames_per_tick=2, generation_settings=gs)
    try:
        def run(text=SHORT, voice="nova", **kw):
            req = sched.submit(text, voice, **kw)
            return np.concatenate(list(sched.iter_chunks(req))), req

        raw0, _ = run(stream=True, **STREAM_KW)
        plain, r0 = run()
        assert sched._stream_conv.lim is None and r0.peak_reduction_db is None
        want_stream, gmin = _stream_model(raw0, DB)
        assert gmin < 1.0
        alone, _ = run(stream=True, peak_limit_db=DB, **STREAM_KW)
        assert sched._stream_conv.lim is not None and np.array_equal(_bits(alone), _bits(want_stream))
        # more requests than slots, every other one limited: a reused slot's next tenant that does not ask is not limited
        reqs = [sched.submit(SHORT, "nova", stream=True, **(dict(peak_limit_db=DB) if i % 2 == 0 else {}), **STREAM_KW) for i in range(5)]
        outs = [np.concatenate(list(sched.iter_chunks(r))) for r in reqs]
        for i, o in enumerate(outs):
            assert np.array_equal(_bits(o), _bits(want_stream if i % 2 == 0 else raw0)), i
        # blocking through the scheduler: whole, last, with the uncapped loudness gain
        block, rb = run(loudness=LOUD, peak_limit_db=DB)
        level, g = loudness.normalize(plain, LOUD, cap=False)
        want, gm = LM.limit(level, DB)
        assert np.array_equal(_bits(block), _bits(want)) and rb.peak_reduction_db == LM.reduction_db(gm) > 0.0
        assert rb.loudness_gain_db == loudness.gain_db(g)
        assert np.array_equal(_bits(run()[0]), _bits(plain))
        with pytest.raises(ValueError, match="peak_limit_db"):
            sched.submit(SHORT, "nova", peak_limit_db=True)

        c = TestClient(create_app(tts, settings={}, scheduler=sched))
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "loudness": LOUD, "peak_limit_db": DB})
        assert r.status_code == 200 and r.headers["x-peak-reduction-db"] == f"{LM.reduction_db(gm):.2f}" and r.content == pcm_to_wav_bytes(want, 24000)
        assert r.headers["x-loudness-gain-db"] == f"{loudness.gain_db(g):.2f}"
        r = c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova"})
        assert r.status_code == 200 and "x-peak-reduction-db" not in r.headers and r.content == pcm_to_wav_bytes(plain, 24000)
        for bad in (0.5, -12.5):
            assert c.post("/v1/audio/speech", json={"input": SHORT, "voice": "nova", "peak_limit_db": bad}).status_code == 400
            assert c.post("/v1/text-to-speech/nova/stream", json={"text": SHORT, "peak_limit_db": bad}).status_code == 400
        c = TestClient(create_app(tts, settings={"peak_limit_db": DB, "loudness": LOUD}, scheduler=sched))  # the server's default
        r = c.post("/v1/text-to-speech/nova", json={"text": SHORT})
        assert r.status_code == 200 and r.headers["x-peak-reduction-db"] == f"{LM.reduction_db(gm):.2f}" and r.content == pcm_to_wav_bytes(want, 24000)
        r = c.post("/v1/text-to-speech/nova", json={"text": SHORT, "peak_limit_db": None, "loudness": None})
        assert r.status_code == 200 and "x-peak-reduction-db" not in r.headers and r.content == pcm_to_wav_bytes(plain, 24000)
    finally:
        sched.close()

    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, FRAMES), devices=[0], start_method="forkserver")
    try:
        r = pool.submit(SHORT, "nova", loudness=LOUD, peak_limit_db=DB)
        got = np.concatenate(list(pool.iter_chunks(r)))
        assert r.peak_reduction_db is not None and abs(r.peak_reduction_db - LM.reduction_db(gm)) < 0.01 and r.peak_reduction_db > 0.0
        assert got.shape == want.shape and float(np.sqrt(np.mean((got - want) ** 2))) <= 1e-5
        assert float(np.abs(got).max()) <= LM.ceiling_of_db(DB) * (1.0 + 2.0 ** -23)
        r = pool.submit(SHORT, "nova")
        assert np.concatenate(list(pool.iter_chunks(r))).shape == plain.shape and r.peak_reduction_db is None
        with pytest.raises(ValueError, match="peak_limit_db"):
            pool.submit(SHORT, "nova", peak_limit_db=-13.0)
    finally:
        pool.close()
