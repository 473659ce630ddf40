"""FLAC framing without a GPU: the numpy model (smoltts_amd/flac.py) against the independent decoder (flac_decode_helpers.py),
its stream blocking and subframe choices, the OpenAI route's flac / pcm answers on a stand-in model, and the validation of
``container`` in front of the GPU."""
import numpy as np
import pytest

from flac_decode_helpers import BitReader, crc8, crc16, decode, decode_frame, decode_mono16

from smoltts_amd import flac


def test_decoder_self_checks():
    assert crc8(b"123456789") == 0xF4 and crc16(b"123456789") == 0xFEE8
    # hand-assembled frames: variable blocking, sample number 0, 24 kHz, mono, 16 bits
    def frame(block_code, ext, sub):
        head = bytes([0xFF, 0xF9, block_code << 4 | 0x7, 0x08, 0x00]) + ext
        body = head + bytes([crc8(head)]) + sub
        return body + crc16(body).to_bytes(2, "big")

    const = frame(0b0110, bytes([3]), bytes([0x00]) + (-1234 & 0xFFFF).to_bytes(2, "big"))
    fr = decode_frame(const, 0, None)
    assert fr.kinds == ["constant"] and fr.samples[0].tolist() == [-1234] * 4 and fr.length == len(const)
    vals = [1, -2, 32767, -32768]
    verb = frame(0b0110, bytes([3]), bytes([0x02]) + b"".join((v & 0xFFFF).to_bytes(2, "big") for v in vals))
    fr = decode_frame(verb, 0, None)
    assert fr.kinds == ["verbatim"] and fr.samples[0].tolist() == vals
    bad = bytearray(verb)
    bad[-3] ^= 1
    with pytest.raises(ValueError):
        decode_frame(bytes(bad), 0, None)
    assert BitReader(bytes([0b10110000])).u(3) == 0b101


def _signals(n, rng):
    t = np.arange(n)
    yield "silence", np.zeros(n, np.int16)
    yield "+full", np.full(n, 32767, np.int16)
    yield "-full", np.full(n, -32768, np.int16)
    yield "alternating", np.where(t % 2 == 0, 32767, -32768).astype(np.int16)
    yield "sine", np.rint(0.5 * 32767 * np.sin(2 * np.pi * 440 * t / 24000)).astype(np.int16)
    yield "noise", rng.integers(-32768, 32768, n).astype(np.int16)
    yield "walk", np.clip(np.cumsum(rng.integers(-700, 701, n)), -32768, 32767).astype(np.int16)


SIZES = list(range(1, 41)) + [64, 128, 256, 512, 1024, 2048, 4096, 77, 191, 192, 255, 257, 575, 1153, 3001, 4095, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_model_round_trips_every_block_size(n):
    rng = np.random.default_rng(n)
    for name, x in _signals(n, rng):
        data = flac.encode_file(x, 24000)
        d = decode(data)
        assert np.array_equal(d.samples[0].astype(np.int16), x), (name, n)
        assert d.info.total == n and d.info.rate == 24000 and d.info.channels == 1 and d.info.bits == 16
        assert d.info.min_block == 16 and d.info.max_block == 4096
        assert d.info.max_frame == max(f.length for f in d.frames) and d.info.min_frame == min(f.length for f in d.frames)
        import hashlib

        assert d.info.md5 == hashlib.md5(x.astype("<i2").tobytes()).digest()
        assert all(max(f.partition_orders) <= 8 for f in d.frames)


@pytest.mark.parametrize("rate", sorted(flac.RATE_CODES))
def test_stream_encoder_random_calls(rate):
    rng = np.random.default_rng(rate)
    enc = flac.StreamEncoder(rate)
    data, fed = [flac.stream_header(rate)], []
    sizes = [0, 3, 12, 0, 1, 5000, 15, 1920, 9000, 0, 7] + list(rng.integers(0, 3000, 12))
    for i, k in enumerate(sizes):
        x = np.clip(np.cumsum(rng.integers(-500, 501, int(k))), -32768, 32767).astype(np.int16)
        fed.append(x)
        data.append(enc.feed(x, last=i == len(sizes) - 1))
    stream = b"".join(data)
    got = decode_mono16(stream)  # (checks variable blocking and contiguous sample numbers)
    assert np.array_equal(got, np.concatenate(fed))
    d = decode(stream)
    assert d.info.rate == rate and d.info.total == 0 and d.info.md5 == bytes(16)
    for f in d.frames[:-1]:
        assert 16 <= f.block_size <= 4096
    assert all(max(f.partition_orders) <= 8 for f in d.frames)


def test_hold_back_at_most_15():
    enc = flac.StreamEncoder(24000)
    assert enc.feed(np.arange(15, dtype=np.int16)) == b""
    out = enc.feed(np.arange(1, dtype=np.int16))
    assert out and decode_frame(out, 0, None).block_size == 16
    assert enc.feed(np.zeros(0, np.int16), last=True) == b""
    assert flac.block_sizes(8193, False) == [2731, 2731, 2731] and flac.block_sizes(4097, False) == [2049, 2048]
    assert flac.block_sizes(3, True) == [3] and flac.block_sizes(3, False) == []


def test_subframe_choices_and_compression():
    def kinds(x, rate=24000):
        return [k for f in decode(flac.encode_file(x, rate)).frames for k in f.kinds]

    assert set(kinds(np.zeros(4096, np.int16))) == {"constant"}
    rng = np.random.default_rng(1)
    assert set(kinds(rng.integers(-32768, 32768, 4096).astype(np.int16))) == {"verbatim"}
    t = np.arange(24000)
    sine = np.rint(0.5 * 32767 * np.sin(2 * np.pi * 440 * t / 24000)).astype(np.int16)
    assert all(k.startswith("fixed") for k in kinds(sine))
    assert len(flac.encode_file(sine, 24000)) < 0.4 * sine.nbytes


def test_quantize_rule():
    x = np.array([-2.0, -1.0, -0.5, 0.0, 1.5e-5, 0.5, 1.0, 3.0], np.float32)
    assert flac.quantize(x).tolist() == np.rint(np.clip(x, -1, 1) * np.float32(32767)).astype(np.int16).tolist()


def test_coded_numbers():
    for v in (0, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1FFFFF, 1 << 21, (1 << 31) - 1, 1 << 31, (1 << 36) - 1):
        fr = flac.encode_frame(np.zeros(16, np.int16), v, 24000)
        assert decode_frame(fr, 0, None).number == v


# ------------------------------------------------------------------------------- the OpenAI route on a stand-in model
def _pcm():
    t = np.arange(1920 * 5)
    return (0.3 * np.sin(2 * np.pi * 220 * t / 24000)).astype(np.float32)


class _FlacTTS:
    """Stand-in model: float32 chunks, or the model's FLAC bytes when asked for the container."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", kw))
        return _pcm()

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", kw))
        if text == "too long":
            raise ValueError("prompt of 9999 positions + max_new_tokens > max_seq_len")
        x = _pcm()
        enc = flac.StreamEncoder(24000) if kw.get("container") == "flac" else None
        for i in range(5):
            c = x[1920 * i: 1920 * (i + 1)]
            if enc is None:
                yield c
            else:
                b = enc.feed(flac.quantize(c), last=i == 4)
                yield np.frombuffer((flac.stream_header(24000) if i == 0 else b"") + b, np.uint8)


def _client(model):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model))


def test_openai_flac_streams_lossless():
    m = _FlacTTS()
    r = _client(m).post("/v1/audio/speech", json={"input": "hi", "voice": "alloy", "response_format": "flac"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    assert 'filename="speech.flac"' in r.headers["content-disposition"]
    assert np.array_equal(decode_mono16(r.content), flac.quantize(_pcm()))
    assert m.calls[-1][1].get("container") == "flac"


def test_openai_pcm_streams_int16():
    m = _FlacTTS()
    r = _client(m).post("/v1/audio/speech", json={"input": "hi", "response_format": "pcm"})
    assert r.status_code == 200 and 'filename="speech.pcm"' in r.headers["content-disposition"]
    assert r.content == flac.quantize(_pcm()).astype("<i2").tobytes()
    assert "container" not in m.calls[-1][1]


@pytest.mark.parametrize("fmt", ["flac", "pcm"])
def test_openai_stream_refusal_is_400_before_any_byte(fmt):
    r = _client(_FlacTTS()).post("/v1/audio/speech", json={"input": "too long", "response_format": fmt})
    assert r.status_code == 400 and "max_seq_len" in r.json()["detail"]


def test_openai_wav_unchanged():
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    m = _FlacTTS()
    r = _client(m).post("/v1/audio/speech", json={"input": "hi"})
    assert r.status_code == 200 and r.content == pcm_to_wav_bytes(_pcm(), 24000) and m.calls[-1][0] == "call"
    assert _client(m).post("/v1/audio/speech", json={"input": "hi", "response_format": "mp3"}).status_code == 422


def test_container_validation_in_front_of_the_gpu():
    from smoltts_amd.formats import check_container
    from smoltts_amd.server.pool import GpuPool
    from smoltts_amd.server.scheduler import BatchScheduler

    assert check_container(None) is None and check_container("flac", "pcm_16000") == "flac"
    for bad in [dict(container="ogg", stream=True), dict(container="flac", stream=False),
                dict(container="flac", stream=True, output_format="ulaw_8000")]:
        pool = GpuPool.__new__(GpuPool)  # (no workers: refused before any is chosen)
        with pytest.raises(ValueError):
            GpuPool.submit(pool, "x", **bad)
        sched = BatchScheduler.__new__(BatchScheduler)  # (refused before the scheduler's state is touched)
        with pytest.raises(ValueError):
            BatchScheduler.submit(sched, "x", **bad)


def test_format_names_stay_refused():
    from smoltts_amd.formats import parse_stream_format

    for name in ("flac_8000", "flac_24000"):
        with pytest.raises(ValueError):
            parse_stream_format(name)
