"""Per-request speaking speed, host side (no GPU): the speed parser, the numpy WSOLA model (tsm.py) that the GPU kernel is
checked against, and the speech routes with a stand-in model that applies the model."""
import math

import numpy as np
import pytest

from smoltts_amd import tsm


def test_speed_validation_and_q16():
    assert tsm.speed_q(1.0) == 65536 and tsm.speed_q(0.25) == 16384 and tsm.speed_q(4.0) == 262144
    assert tsm.speed_q(0.3) == 19661 and tsm.speed_q(1.5) == 98304 and tsm.speed_q("2") == 131072
    assert tsm.speed_q(1.00001) == 65537  # (round half away: 65536.655 -> 65537)
    assert tsm.parse_speed(None) is None and tsm.parse_speed(1.0) is None and tsm.parse_speed(1.000001) is None
    assert tsm.parse_speed(2.0) == 131072
    for bad in (0.1, 0.2499, 4.0001, 5, -1, float("nan"), float("inf"), "fast", None):
        with pytest.raises(ValueError):
            tsm.speed_q(bad)


def test_identity_at_speed_one():
    x = np.random.default_rng(0).standard_normal(5000).astype(np.float32) * 0.1
    y = tsm.stretch(x, 1.0)
    assert y.dtype == np.float32 and np.array_equal(y, x)
    with pytest.raises(ValueError):
        tsm.Stretcher(65535 * 5)
    assert np.array_equal(tsm.stretch(x, speed_q=131072), tsm.stretch(x, 2.0))
    with pytest.raises(ValueError, match=r"\[0.25, 4.0\]"):
        tsm.stretch(x, 5)  # a factor out of range, not a Q16 value
    with pytest.raises(ValueError):
        tsm.stretch(x)
    with pytest.raises(ValueError):
        tsm.stretch(x, 2.0, speed_q=131072)


def _voiced(n, seed=0, f0=150.0):
    """A speech-like test signal: a harmonic tone with a slow vibrato, an amplitude envelope and a little noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.03 * np.sin(2 * np.pi * 3 * t))) / 24000.0
    x = sum(0.3 / k * np.sin(k * ph) for k in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * t))
    return (x + 0.01 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("speed", [0.25, 0.5, 0.8, 1.25, 2.0, 4.0])
def test_output_length_is_exactly_m(speed):
    sq = tsm.speed_q(speed)
    for n in (0, 1, 239, 240, 700, 1920, 4801, 12345):
        y = tsm.stretch(_voiced(n, n), speed)
        assert y.shape == (math.ceil(n * 65536 / sq),) == (tsm.out_length(n, sq),), (speed, n)


@pytest.mark.parametrize("speed", [0.25, 0.8, 2.0, 4.0])
def test_streaming_equals_whole_signal(speed):
    sq = tsm.speed_q(speed)
    x = _voiced(24000, 3)
    want, pos = tsm.stretch(x, speed, return_positions=True)
    assert pos[0] == 0 and all(p >= 0 for p in pos)
    rng = np.random.default_rng(int(speed * 100))
    plans = {"1920": [1920] * 13, "7680": [7680] * 4, "random": []}
    n = 0
    while n < x.size:
        plans["random"].append(int(rng.integers(1, 4000)))
        n += plans["random"][-1]
    for name, sizes in plans.items():
        got, outs = tsm.stream_chunks(x, sq, sizes)
        assert np.array_equal(got, want), name
        assert sum(o.size for o in outs) == want.size
    x1 = x[:3000]  # one sample per call
    got, _ = tsm.stream_chunks(x1, sq, [1] * x1.size)
    assert np.array_equal(got, tsm.stretch(x1, speed))


def test_first_chunk_lookahead_at_speed_one_ish():
    # the first 1920-sample frame releases 6 segments (a_5 + 192 + 480 <= 1920): 1440 samples
    st = tsm.Stretcher(tsm.speed_q(1.0 + 1 / 65536))
    assert st.push(_voiced(1920)).size == 1440


def _dominant_hz(y):
    w = np.hanning(y.size)
    spec = np.abs(np.fft.rfft(y * w))
    spec[: int(50 * y.size / 24000)] = 0
    return float(np.argmax(spec)) * 24000.0 / y.size


@pytest.mark.parametrize("speed", [0.5, 2.0])
def test_pitch_is_kept_and_duration_scales(speed):
    t = np.arange(48000) / 24000.0
    x = sum(0.25 / k * np.sin(2 * np.pi * 150 * k * t) for k in range(1, 5)).astype(np.float32)
    y = tsm.stretch(x, speed)
    assert y.size == tsm.out_length(x.size, tsm.speed_q(speed))
    assert abs(y.size / x.size - 1 / speed) < 1e-3
    core = y[y.size // 8: -y.size // 8]
    assert abs(_dominant_hz(core) - 150.0) <= 0.02 * 150.0
    # plain resampling would have moved it to 150 * speed
    assert abs(_dominant_hz(core) - 150.0 * speed) > 0.2 * 150.0


def test_tie_rule_on_a_period_dividing_the_hop():
    """Period 60 divides L = 240: lags 60 apart are exact matches.  At speed 1.125 (a_k steps by 270 = 4.5 periods) the lags
    +30 and -30 tie at D = 0 every other segment; the rule picks the smaller |delta|, then the negative one."""
    period = (0.5 * np.sin(2 * np.pi * np.arange(60) / 60)).astype(np.float32)
    x = np.tile(period, 200)
    sq = tsm.speed_q(1.125)
    _, pos = tsm.stretch(x, speed_q=sq, return_positions=True)
    q = tsm.to_s16(np.concatenate([x, np.zeros(2048, np.float32)]))
    ties = 0
    for k in range(1, len(pos)):
        a = tsm.nominal(k, sq)
        ref = q[pos[k - 1] + tsm.L: pos[k - 1] + 2 * tsm.L]
        scored = []
        for d in range(-tsm.DELTA, tsm.DELTA + 1):
            if a + d >= 0:
                scored.append((int(np.abs(q[a + d: a + d + tsm.L] - ref).sum()), abs(d), d))
        scored.sort()
        assert pos[k] == a + scored[0][2], k
        if scored[0][0] == scored[1][0] and scored[0][1] == scored[1][1] and scored[0][1] > 0:
            ties += 1
            assert pos[k] - a < 0
    assert ties >= 10


# ---------------------------------------------------------------------------------------------------- routes
class _SpeedTTS:
    """Stand-in model: applies the numpy model for a speed; records what it was called with."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def _pcm(self):
        return _voiced(1920 * 6, 9)

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", kw.get("speed")))
        x = self._pcm()
        return tsm.stretch(x, kw["speed"]) if "speed" in kw else x

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", kw.get("speed")))
        st = tsm.Stretcher(tsm.speed_q(kw["speed"])) if "speed" in kw else None
        x = self._pcm()
        for i in range(6):
            c = x[1920 * i: 1920 * (i + 1)]
            c = st.push(c, last=i == 5) if st is not None else c
            if c.size:
                yield c


class _PlainTTS(_SpeedTTS):
    """The model as it was: no speed argument at all."""

    def __call__(self, text, voice="heart"):
        return self._pcm()

    def stream(self, text, voice="heart"):
        x = self._pcm()
        for i in range(6):
            yield x[1920 * i: 1920 * (i + 1)]


def _client(model):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model))


def test_openai_speed_two_halves_the_audio():
    model = _SpeedTTS()
    c = _client(model)
    r = c.post("/v1/audio/speech", json={"input": "quick", "voice": "sky", "speed": 2.0})
    assert r.status_code == 200 and r.content[:4] == b"RIFF"
    n = np.frombuffer(r.content[44:], np.int16).size
    assert n == tsm.out_length(1920 * 6, 131072) == 5760
    assert model.calls == [("call", 2.0)]
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    assert r.content == pcm_to_wav_bytes(tsm.stretch(model._pcm(), 2.0), 24000)


def test_elevenlabs_voice_settings_speed_blocking_and_stream():
    model = _SpeedTTS()
    c = _client(model)
    body = {"text": "slowly", "voice_settings": {"speed": 0.5, "stability": 0.3, "similarity_boost": 0.8}}
    r = c.post("/v1/text-to-speech/sky?output_format=pcm_24000", json=body)
    assert r.status_code == 200
    assert np.frombuffer(r.content, np.int16).size == tsm.out_length(1920 * 6, 32768)
    r = c.post("/v1/text-to-speech/sky/stream", json=body)
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "24000"
    got = np.frombuffer(r.content, np.float32)
    assert np.array_equal(got, tsm.stretch(model._pcm(), 0.5))
    # voice_settings without a speed, and speed 1.0, reach the model as no speed at all
    assert c.post("/v1/text-to-speech/sky/stream", json={"text": "x", "voice_settings": {"stability": 0.5}}).status_code == 200
    assert c.post("/v1/audio/speech", json={"input": "x", "speed": 1.0}).status_code == 200
    assert model.calls == [("call", 0.5), ("stream", 0.5), ("stream", None), ("call", None)]


@pytest.mark.parametrize("bad", ["0.1", "5", "NaN", "Infinity", '"quick"'])
def test_out_of_range_speed_is_422_on_every_route(bad):
    model = _SpeedTTS()
    c = _client(model)
    hdr = {"content-type": "application/json"}  # (raw bodies: NaN is not JSON an encoder would write, but clients send it)
    assert c.post("/v1/audio/speech", content='{"input": "x", "speed": %s}' % bad, headers=hdr).status_code == 422
    for route in ("/v1/text-to-speech/sky", "/v1/text-to-speech/sky/stream"):
        body = '{"text": "x", "voice_settings": {"speed": %s}}' % bad
        assert c.post(route, content=body, headers=hdr).status_code == 422, route
    assert model.calls == []


def test_no_speed_gives_todays_bytes():
    """A model without any speed argument serves every route as before: the routes pass nothing new."""
    model = _PlainTTS()
    c = _client(model)
    x = model._pcm()
    r = c.post("/v1/audio/speech", json={"input": "x", "voice": "sky"})
    assert r.status_code == 200
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    assert r.content == pcm_to_wav_bytes(x, 24000)
    r = c.post("/v1/text-to-speech/sky?output_format=pcm_24000", json={"text": "x", "voice_settings": {"speed": 1.0}})
    assert r.content == np.rint(np.clip(x, -1, 1) * 32767).astype(np.int16).tobytes()
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "x"})
    assert r.content == x.tobytes()


def test_pool_refuses_a_bad_speed_in_the_parent():
    from smoltts_amd.server.pool import GpuPool

    pool = GpuPool.__new__(GpuPool)  # (no workers: the speed is refused before any is chosen)
    for bad in (0.1, 4.5, float("nan")):
        with pytest.raises(ValueError):
            GpuPool.submit(pool, "x", speed=bad)


def test_null_speed_is_speed_one():
    """An explicit null (clients that send every setting, unset ones as null) is answered as before: no speed."""
    model = _SpeedTTS()
    c = _client(model)
    assert c.post("/v1/audio/speech", json={"input": "x", "speed": None}).status_code == 200
    assert c.post("/v1/text-to-speech/sky", json={"text": "x", "voice_settings": {"speed": None}}).status_code == 200
    assert c.post("/v1/text-to-speech/sky/stream", json={"text": "x", "voice_settings": None}).status_code == 200
    assert model.calls == [("call", None), ("call", None), ("stream", None)]


def test_stream_end_rule_same_on_numpy_and_torch():
    """The scheduler closes a stream on the host and flushes its stretcher on the device with ``stream_ends``: the two must
    agree for every snapshot."""
    import torch

    from smoltts_amd.server.scheduler import stream_ends

    n, done, cap = (a.ravel() for a in np.meshgrid(np.arange(8), np.arange(3), np.arange(7), indexing="ij"))
    n, done, cap = n.astype(np.int32), done.astype(np.int32), cap.astype(np.int32)
    host = stream_ends(n, done, cap)
    dev = stream_ends(torch.from_numpy(n), torch.from_numpy(done), torch.from_numpy(cap))
    assert host.dtype == np.bool_ and dev.dtype == torch.bool
    assert np.array_equal(host, dev.numpy())
    for i in range(n.size):  # one slot of a snapshot, as _drain reads it: stopped with a frame, or the budget reached
        want = (bool(done[i]) and int(n[i]) > 0) or min(int(n[i]), int(cap[i])) >= int(cap[i])
        assert bool(stream_ends(n[i], done[i], int(cap[i]))) == bool(host[i]) == want
