"""Cloned voices end to end over HTTP: POST /v1/voices/add with base64 WAV at 48 and 16 kHz, then the voice_id on the speech
routes, on a scheduler and on a two-worker pool; the audio must equal the façade's with speaker=create_speaker(...) of the same
samples resampled to 24 kHz by scipy.signal.resample_poly."""
import base64
import functools

import numpy as np
import pytest
from scipy.signal import resample_poly

from voice_helpers import wav_bytes

pytestmark = pytest.mark.gpu

RATIO = {48000: (1, 2), 16000: (3, 2)}


def _uploads():
    """Two samples: 16-bit stereo at 48 kHz and float mono at 16 kHz -> (request JSON samples, the 24 kHz audio they decode to)."""
    from smoltts_amd.codec.synthetic import synthetic_pcm

    a = synthetic_pcm(2 * 1920 * 3, 11) * 0.5
    st = np.stack([a, a[::-1]], 1)
    s16 = np.rint(np.clip(st, -1, 1) * 32767).astype(np.int16)
    b = (synthetic_pcm(1920 * 2 // 3 * 2, 12) * 0.5).astype(np.float32)
    body = [{"text": "the first reference line", "audio": base64.b64encode(wav_bytes(s16, 48000)).decode()},
            {"text": "a second one", "audio": base64.b64encode(wav_bytes(b, 16000, "float")).decode()}]
    pcm = [resample_poly((s16.astype(np.float64) / 32768.0).mean(axis=1), *RATIO[48000]).astype(np.float32),
           resample_poly(b.astype(np.float64), *RATIO[16000]).astype(np.float32)]
    return body, [{"text": x["text"], "audio": p} for x, p in zip(body, pcm)]


def _rms(g, w):
    return float(np.sqrt(np.mean((g.astype(np.float64) - w) ** 2)))


def _tts():
    from smoltts_amd import SmolTTS
    from smoltts_amd.codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state
    from smoltts_amd.synthetic import named_config, synthetic_lm_state

    cfg = named_config("tiny")
    return SmolTTS(state=synthetic_lm_state(cfg, seed=21), config=cfg, mimi_state={**synthetic_mimi_state(seed=5), **synthetic_mimi_encoder_state(seed=5)})


def _check_routes(client, tts, n):
    from smoltts_amd.config import GenerationSettings

    body, samples = _uploads()
    r = client.post("/v1/voices/add", json={"name": "narrator", "samples": body})
    assert r.status_code == 200, r.text
    vid = r.json()["voice_id"]
    spk = tts.create_speaker(samples)
    listed = [v for v in client.get("/v1/voices").json()["voices"] if v["voice_id"] == vid]
    assert listed == [{"voice_id": vid, "name": "narrator", "category": "cloned", "prompt_positions": int(spk.shape[1])}]
    gs = GenerationSettings.greedy(max_new_tokens=n)
    want = tts("spoken in the cloned voice", None, speaker=spk, generation_settings=gs)
    tts.add_voice("cv_reference", spk)
    try:
        want_stream = np.concatenate(list(tts.stream("spoken in the cloned voice", "cv_reference", generation_settings=gs)))
    finally:
        tts.remove_voice("cv_reference")
    resp = client.post(f"/v1/text-to-speech/{vid}/stream", json={"text": "spoken in the cloned voice"})
    assert resp.status_code == 200
    got = np.frombuffer(resp.content, dtype=np.float32)
    assert got.shape == want_stream.shape and _rms(got, want_stream) <= 1e-6
    resp = client.post(f"/v1/text-to-speech/{vid}?output_format=pcm_24000", json={"text": "spoken in the cloned voice"})
    assert resp.status_code == 200
    pcm16 = np.frombuffer(resp.content, dtype=np.int16)
    ref16 = np.rint(np.clip(want, -1, 1) * 32767).astype(np.int16)
    assert pcm16.shape == ref16.shape and int(np.abs(pcm16.astype(np.int32) - ref16.astype(np.int32)).max()) <= 1
    resp = client.post("/v1/audio/speech", json={"input": "spoken in the cloned voice", "voice": vid})
    assert resp.status_code == 200 and resp.content[:4] == b"RIFF"
    assert np.frombuffer(resp.content[44:], dtype=np.int16).shape == ref16.shape
    assert client.delete(f"/v1/voices/{vid}").status_code == 200
    assert client.delete(f"/v1/voices/{vid}").status_code == 404


def test_voice_routes_on_a_scheduler():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.config import GenerationSettings
    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.scheduler import BatchScheduler

    tts = _tts()
    sched = BatchScheduler(tts, max_batch=4, frames_per_tick=2, generation_settings=GenerationSettings.greedy(max_new_tokens=16),
                           prefill_chunk=8)
    try:
        _check_routes(TestClient(create_app(tts, {}, sched)), tts, 16)
        assert sched.stats()["prefix_installs"] == 3
    finally:
        sched.close()


def test_voice_routes_on_a_pool_of_two_workers():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app
    from smoltts_amd.server.pool import GpuPool, synthetic_scheduler

    pool = GpuPool(functools.partial(synthetic_scheduler, "tiny", 21, 5, 2, 2, 16, mimi_encoder=True), devices=[0, 0],
                   start_method="forkserver")
    try:
        _check_routes(TestClient(create_app(None, {}, pool)), _tts(), 16)
    finally:
        pool.close()
