"""Cloned voices without a GPU: WAV decoding and resampling of uploaded samples, the voice routes over stand-in schedulers and
models, and the pool's voice registry protocol with stand-in workers."""
import base64
import functools
import threading
import time

import numpy as np
import pytest
from scipy.signal import resample_poly

from voice_helpers import make_voice_echo, wav_bytes

RATES = (8000, 16000, 22050, 24000, 44100, 48000)


def _b64(b: bytes) -> str:
    return base64.b64encode(b).decode()


# ------------------------------------------------------------------ WAV decoding
@pytest.mark.parametrize("rate", RATES)
def test_wav_every_rate_equals_resample_poly(rate):
    from smoltts_amd.server.voices import decode_sample_audio, parse_wav

    rng = np.random.default_rng(rate)
    s16 = rng.integers(-20000, 20000, size=rate // 10, dtype=np.int16)
    x, r = parse_wav(wav_bytes(s16, rate))
    assert r == rate and x.dtype == np.float64 and np.array_equal(x, s16.astype(np.float64) / 32768.0)
    got = decode_sample_audio(_b64(wav_bytes(s16, rate)))
    if rate == 24000:
        want = (s16.astype(np.float64) / 32768.0).astype(np.float32)
    else:
        from math import gcd

        g = gcd(24000, rate)
        want = resample_poly(s16.astype(np.float64) / 32768.0, 24000 // g, rate // g).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize("kind", ["pcm16", "float"])
@pytest.mark.parametrize("extensible", [False, True])
def test_wav_stereo_float_and_extensible(kind, extensible):
    from smoltts_amd.server.voices import decode_sample_audio, parse_wav

    rng = np.random.default_rng(3)
    if kind == "pcm16":
        st = rng.integers(-30000, 30000, size=(4410, 2), dtype=np.int16)
        dec = st.astype(np.float64) / 32768.0
    else:
        st = rng.uniform(-0.9, 0.9, size=(4410, 2)).astype(np.float32)
        dec = st.astype(np.float64)
    x, r = parse_wav(wav_bytes(st, 44100, kind, extensible))
    assert r == 44100 and np.array_equal(x, dec.mean(axis=1))
    got = decode_sample_audio(_b64(wav_bytes(st, 44100, kind, extensible)))
    assert np.array_equal(got, resample_poly(dec.mean(axis=1), 80, 147).astype(np.float32))
    # three channels, averaged
    x3, _ = parse_wav(wav_bytes(np.stack([st[:, 0], st[:, 1], st[:, 0]], 1), 16000, kind, extensible))
    assert np.allclose(x3, (2 * dec[:, 0] + dec[:, 1]) / 3, rtol=0, atol=1e-15)


def test_wav_corrupt_and_unsupported_inputs_raise():
    import struct

    from smoltts_amd.server.voices import decode_sample_audio, parse_wav

    good = wav_bytes(np.zeros(100, np.int16), 16000)
    bad = [b"", b"RIFF1234WAVX", good[:20], good.replace(b"fmt ", b"fmt_"),  # no fmt chunk
           wav_bytes(np.zeros(100, np.int16), 11025),  # unsupported rate
           wav_bytes(np.zeros(0, np.int16), 16000)]  # no samples
    # 8-bit PCM, 24-bit PCM, 64-bit float: unsupported sample formats
    for code, bits in ((1, 8), (1, 24), (3, 64), (6, 8)):
        b = bytearray(good)
        i = b.index(b"fmt ") + 8
        blk = bits // 8
        b[i: i + 16] = struct.pack("<HHIIHH", code, 1, 16000, 16000 * blk, blk, bits)
        bad.append(bytes(b))
    for b in bad:
        with pytest.raises(ValueError):
            parse_wav(b)
    for s in ("not base64!!", _b64(b"RIFF....WAVE"), "QUJD=="[:5]):
        with pytest.raises(ValueError):
            decode_sample_audio(s)


def test_voice_ids_never_collide_with_presets():
    from smoltts_amd.prompt import VOICE_MAP
    from smoltts_amd.server.voices import new_voice_id

    ids = {new_voice_id() for _ in range(2000)}
    assert len(ids) == 2000
    for v in ids:
        assert v.startswith("cv_") and len(v) == 23 and int(v[3:], 16) >= 0
        assert v not in VOICE_MAP and not v.isnumeric()


# ------------------------------------------------------------------ routes
class _FakeScheduler:
    """BatchScheduler stand-in: records what reaches submit; add_voice refuses by the sample text."""

    def __init__(self):
        self.submitted = []
        self.voices = {}

    def submit(self, text, voice="heart", stream=False, max_new_tokens=None, output_format=None, sampling=None):
        self.submitted.append((text, voice, stream, output_format))
        q = [np.zeros(1920, np.float32) if output_format is None else np.zeros(1920, np.int16), None]

        class R:
            pass

        r = R()
        r.items, r.sampling = q, sampling
        return r

    def iter_chunks(self, r):
        for it in r.items:
            if it is None:
                return
            yield it

    def add_voice(self, voice_id, samples=None, grid=None, system_prompt=None, name=None):
        from smoltts_amd import NoEncoderError

        t = samples[0]["text"]
        if t == "no encoder":
            raise NoEncoderError("the Mimi checkpoint has no encoder.* weights")
        if t == "too long":
            raise ValueError("speaker prompt of P=900 positions leaves no room for a request: ... > max_seq_len 512")
        if t == "encoder limit":
            raise ValueError("cannot encode the samples: beyond the encoder's positions")
        assert samples[0]["audio"].dtype == np.float32
        self.voices[voice_id] = samples
        return {"voice_id": voice_id, "prompt_positions": 40}

    def remove_voice(self, voice_id):
        del self.voices[voice_id]


def _client(sched=None, model=None, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model, settings, sched))


def _sample(text="hello there", rate=16000, n=1600):
    return {"text": text, "audio": _b64(wav_bytes(np.zeros(n, np.int16), rate))}


def test_voice_routes_on_a_scheduler():
    sched = _FakeScheduler()
    c = _client(sched)
    r = c.post("/v1/voices/add", json={"name": "narrator", "samples": [_sample(), _sample("second", 48000)], "system_prompt": None})
    assert r.status_code == 200, r.text
    vid = r.json()["voice_id"]
    assert vid.startswith("cv_") and len(vid) == 23 and vid in sched.voices
    assert [s["text"] for s in sched.voices[vid]] == ["hello there", "second"]
    assert sched.voices[vid][1]["audio"].shape == (800,)  # 1600 samples at 48 kHz -> 24 kHz
    lst = c.get("/v1/voices").json()["voices"]
    assert {"voice_id": "heart", "name": "heart", "category": "premade"} in lst
    assert {"voice_id": vid, "name": "narrator", "category": "cloned", "prompt_positions": 40} in lst
    # the id reaches submit on every speech route
    assert c.post("/v1/audio/speech", json={"input": "a", "voice": vid}).status_code == 200
    assert c.post(f"/v1/text-to-speech/{vid}", json={"text": "b"}).status_code == 200
    assert c.post(f"/v1/text-to-speech/{vid}/stream", json={"text": "c"}).status_code == 200
    assert c.post(f"/v1/text-to-speech/{vid}/stream?output_format=pcm_16000", json={"text": "d"}).status_code == 200
    assert [s[:2] for s in sched.submitted] == [("a", vid), ("b", vid), ("c", vid), ("d", vid)]
    assert sched.submitted[3][3] == "pcm_16000"
    # delete: 200, then 404; a premade voice cannot be deleted
    assert c.delete(f"/v1/voices/{vid}").status_code == 200 and vid not in sched.voices
    assert c.delete(f"/v1/voices/{vid}").status_code == 404
    assert c.delete("/v1/voices/cv_00000000000000000000").status_code == 404
    assert c.delete("/v1/voices/heart").status_code == 400
    assert all(v["category"] == "premade" for v in c.get("/v1/voices").json()["voices"])


def test_voice_route_errors():
    sched = _FakeScheduler()
    c = _client(sched, settings={"max_voices": 2})
    add = lambda samples: c.post("/v1/voices/add", json={"name": "x", "samples": samples})  # noqa: E731
    assert add([{"text": "t", "audio": "***"}]).status_code == 400                            # bad base64
    assert add([{"text": "t", "audio": _b64(b"RIFF0000WAVEjunk")}]).status_code == 400        # bad WAV
    assert add([_sample(rate=11025)]).status_code == 400                                       # unsupported rate
    assert add([{"audio": _sample()["audio"]}]).status_code == 400                            # no text
    assert add([_sample(text="  ")]).status_code == 400
    r = add([_sample(text="too long")])
    assert r.status_code == 400 and "max_seq_len" in r.json()["detail"] and "P=900" in r.json()["detail"]
    assert add([_sample(text="encoder limit")]).status_code == 400
    assert add([_sample(text="no encoder")]).status_code == 501
    assert add([]).status_code == 422
    assert not sched.voices and c.get("/v1/voices").json()["voices"][-1]["category"] == "premade"
    assert add([_sample()]).status_code == 200 and add([_sample()]).status_code == 200
    assert add([_sample()]).status_code == 409  # max_voices
    assert len(sched.voices) == 2


class _FakeModel:
    """SmolTTS stand-in for create_app(model): create_speaker + add_voice, and what reaches __call__ / stream."""

    def __init__(self, encoder=True):
        self.voices, self.calls, self.encoder = {}, [], encoder

    def create_speaker(self, samples, system_prompt=None):
        from smoltts_amd import NoEncoderError

        if not self.encoder:
            raise NoEncoderError("the Mimi checkpoint has no encoder.* weights")
        return np.zeros((9, 10 + len(samples)), np.int32)

    def add_voice(self, voice_id, grid):
        self.voices[voice_id] = grid

    def remove_voice(self, voice_id):
        del self.voices[voice_id]

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", text, voice))
        return np.zeros(1920, np.float32)

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", text, voice))
        yield np.zeros(1920, np.float32)


def test_voice_routes_on_the_model_only_path():
    m = _FakeModel()
    c = _client(model=m)
    r = c.post("/v1/voices/add", json={"name": "n", "samples": [_sample(), _sample()]})
    assert r.status_code == 200
    vid = r.json()["voice_id"]
    assert m.voices[vid].shape == (9, 12)
    assert {"voice_id": vid, "name": "n", "category": "cloned", "prompt_positions": 12} in c.get("/v1/voices").json()["voices"]
    assert c.post("/v1/audio/speech", json={"input": "a", "voice": vid}).status_code == 200
    assert c.post(f"/v1/text-to-speech/{vid}", json={"text": "b"}).status_code == 200
    assert c.post(f"/v1/text-to-speech/{vid}/stream", json={"text": "c"}).status_code == 200
    assert [x[2] for x in m.calls] == [vid] * 3
    assert c.delete(f"/v1/voices/{vid}").status_code == 200 and not m.voices
    c2 = _client(model=_FakeModel(encoder=False))
    assert c2.post("/v1/voices/add", json={"name": "n", "samples": [_sample()]}).status_code == 501


def test_max_voices_setting():
    from smoltts_amd.server.settings import ServerSettings

    assert ServerSettings(checkpoint_dir="/x").max_voices == 64
    assert ServerSettings(checkpoint_dir="/x", max_voices=3).model_dump()["max_voices"] == 3


# ------------------------------------------------------------------ pool protocol
@pytest.fixture()
def _no_mask(monkeypatch):
    monkeypatch.delenv("HIP_VISIBLE_DEVICES", raising=False)


def test_pool_broadcasts_voices_and_replays_them(_no_mask):
    from smoltts_amd.server.pool import GpuPool

    pool = GpuPool(functools.partial(make_voice_echo, 0.0), devices=[0, 1], ready_timeout=120)
    try:
        samples = [{"text": "a line", "audio": np.zeros(6, np.float32)}]
        res = pool.add_voice("cv_a", samples=samples, name="A")
        assert res == {"voice_id": "cv_a", "prompt_positions": 3 + 6 % 5}
        assert pool.voices() == {"cv_a": {"name": "A", "prompt_positions": 4}}
        pool.add_voice("cv_b", grid=np.zeros((9, 11), np.int32))
        with pytest.raises(ValueError):
            pool.add_voice("cv_c", samples=[{"text": "", "audio": np.zeros(3)}])
        assert set(pool.voices()) == {"cv_a", "cv_b"}

        def on_both(voice):
            """Two requests at once land on the two workers: -> {device: (known, P)}."""
            seen = {}
            for _ in range(5):
                hold = pool.submit("h" * 2000, voice)
                g = np.stack(list(pool.iter_chunks(pool.submit("abc", voice))))
                h = np.stack(list(pool.iter_chunks(hold)))
                for x in (g, h):
                    seen[int(x[0, 0])] = (int(x[0, 2]), int(x[0, 3]))
                if len(seen) == 2:
                    break
            return seen

        assert on_both("cv_a") == {0: (1, 4), 1: (1, 4)}  # registered everywhere before add_voice returned
        assert on_both("cv_b") == {0: (1, 11), 1: (1, 11)}
        pool.remove_voice("cv_b")
        assert on_both("cv_b") == {0: (0, 0), 1: (0, 0)}
        with pytest.raises(KeyError):
            pool.remove_voice("cv_b")
        assert pool.stats()["in_flight"] == [0, 0]
        # a replaced worker gets the registered voices before it takes requests
        killer = pool.submit("__die__")
        with pytest.raises(RuntimeError, match="died"):
            list(pool.iter_chunks(killer))
        deadline = time.time() + 60
        while pool.stats()["alive"] < 2 and time.time() < deadline:
            time.sleep(0.1)
        assert pool.stats()["restarts"][killer.worker] == 1
        assert on_both("cv_a") == {0: (1, 4), 1: (1, 4)}
    finally:
        pool.close()


def test_pool_voice_routes_end_to_end(_no_mask):
    from smoltts_amd.server.pool import GpuPool

    pool = GpuPool(functools.partial(make_voice_echo, 0.0), devices=[0, 1], ready_timeout=120)
    try:
        c = _client(pool)
        r = c.post("/v1/voices/add", json={"name": "n", "samples": [_sample()]})
        assert r.status_code == 200
        vid = r.json()["voice_id"]
        assert set(pool.voices()) == {vid}
        assert c.post(f"/v1/text-to-speech/{vid}/stream", json={"text": "abc"}).status_code == 200
        assert c.delete(f"/v1/voices/{vid}").status_code == 200 and pool.voices() == {}
    finally:
        pool.close()
