"""Streamed output formats, host side (no GPU): the library's filter design against scipy, the host mu-law against the G.711
formula on every int16, and the HTTP routes with a stand-in model whose ``stream`` takes ``output_format``."""
import numpy as np
import pytest

RATES = {8000: (1, 3), 16000: (2, 3), 22050: (147, 160), 44100: (147, 80), 48000: (2, 1)}


def _ulaw_formula(s: int) -> int:
    sign = 0x80 if s < 0 else 0
    mag = min(abs(s), 32635) + 0x84
    seg = mag.bit_length() - 1 - 7
    mant = (mag >> (seg + 3)) & 0xF
    return ~(sign | (seg << 4) | mant) & 0xFF


@pytest.mark.parametrize("rate", sorted(RATES))
def test_resample_design_matches_scipy(rate):
    signal = pytest.importorskip("scipy.signal")
    from smoltts_amd import engine

    taps, up, down, half = engine.resample_design(rate)
    assert (up, down) == RATES[rate] and half == 10 * max(up, down) and taps.shape == (2 * half + 1,)
    ref = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert np.abs(taps - ref).max() <= 1e-12


def test_resample_design_refuses_other_rates():
    from smoltts_amd import engine

    for rate in (11025, 24000, 0, -8000):
        with pytest.raises(engine.SmolttsError):
            engine.resample_design(rate)


def test_host_ulaw_every_int16():
    from smoltts_amd.formats import lin2ulaw

    s = np.arange(-32768, 32768, dtype=np.int32)
    want = np.array([_ulaw_formula(int(v)) for v in s], np.uint8)
    got = lin2ulaw(s.astype(np.int16))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert lin2ulaw(np.array([0, 32767, -32768], np.int16)).tolist() == [0xFF, 0x80, 0x00]


def test_format_parser():
    from smoltts_amd.formats import ENC_OFF, ENC_S16, ENC_ULAW, parse_stream_format

    assert parse_stream_format("pcm_16000") == (16000, ENC_S16)
    assert parse_stream_format("ulaw_8000") == (8000, ENC_ULAW)
    assert parse_stream_format("pcm_24000") == (24000, ENC_OFF)
    for bad in ("flac_8000", "ulaw_16000", "pcm_11025", "mp3_44100_128", "alaw_8000"):
        with pytest.raises(ValueError, match="pcm_16000"):
            parse_stream_format(bad)


class _FormatTTS:
    """Stand-in model: float32 chunks without a format, otherwise chunks of the format's dtype that encode the request."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def __call__(self, text, voice="heart"):
        return np.sin(np.linspace(0, 40, 1920 * 3)).astype(np.float32) * 0.7

    def stream(self, text, voice="heart", output_format=None):
        self.calls.append(output_format)
        for i in range(3):
            if output_format is None:
                yield np.full(1920, 0.1 * i, dtype=np.float32)
            elif output_format.startswith("ulaw"):
                yield np.full(640, 0x10 + i, dtype=np.uint8)
            else:
                yield np.arange(100, dtype=np.int16) * (i + 1) - 7


@pytest.fixture()
def fmt_client():
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    model = _FormatTTS()
    return TestClient(create_app(model)), model


def test_stream_route_formats(fmt_client):
    client, model = fmt_client
    r = client.post("/v1/text-to-speech/3/stream?output_format=pcm_16000", json={"text": "abc"})
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "16000"
    assert 'filename="speech.pcm"' in r.headers["content-disposition"]
    want = np.concatenate([np.arange(100, dtype=np.int16) * (i + 1) - 7 for i in range(3)])
    assert np.array_equal(np.frombuffer(r.content, dtype="<i2"), want)
    r = client.post("/v1/text-to-speech/3/stream?output_format=ulaw_8000", json={"text": "abc"})
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "8000"
    assert 'filename="speech.ulaw"' in r.headers["content-disposition"]
    assert r.content == bytes([0x10] * 640 + [0x11] * 640 + [0x12] * 640)
    r = client.post("/v1/text-to-speech/3/stream?output_format=pcm_24000", json={"text": "abc"})
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "24000"
    chunks = np.frombuffer(r.content, dtype=np.float32)
    assert chunks.shape == (3 * 1920,) and np.allclose(chunks[1920:1922], 0.1)
    assert model.calls == ["pcm_16000", "ulaw_8000", None]  # pcm_24000 is not passed on
    for bad in ("flac_8000", "ulaw_16000", "pcm_11025"):
        assert client.post(f"/v1/text-to-speech/3/stream?output_format={bad}", json={"text": "abc"}).status_code == 422
    assert len(model.calls) == 3


def test_blocking_ulaw_is_mu_law_of_the_fft_resample(fmt_client):
    signal = pytest.importorskip("scipy.signal")
    from smoltts_amd.formats import lin2ulaw

    client, model = fmt_client
    r = client.post("/v1/text-to-speech/3?output_format=ulaw_8000", json={"text": "abc"})
    assert r.status_code == 200 and r.headers["x-sample-rate"] == "8000"
    pcm = model("abc")
    y = signal.resample(pcm, int(len(pcm) * 8000 / 24000)).astype(np.float32)
    s16 = np.rint(np.clip(y, -1.0, 1.0) * 32767).astype(np.int16)
    assert r.content == lin2ulaw(s16).tobytes()
    assert r.content == bytes(_ulaw_formula(int(v)) for v in s16)
    # the other blocking formats are as they were
    r = client.post("/v1/text-to-speech/3?output_format=pcm_8000", json={"text": "abc"})
    assert r.status_code == 200 and np.array_equal(np.frombuffer(r.content, "<i2"), s16)
