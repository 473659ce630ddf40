"""The watermark's numpy model and detector (``smoltts_amd/watermark.py``), host side: the tables, the model's invariants, detection
through the project's own output paths, the stage's place in ``engine.plan_pass``, and the request, settings and HTTP surface.
No GPU, no library call."""
import base64
import itertools

import numpy as np
import pytest

from smoltts_amd import engine, flac, route, watermark as W
from smoltts_amd.formats import lin2ulaw, parse_stream_format
from smoltts_amd.request import parse_request

from flac_decode_helpers import decode_mono16
from watermark_helpers import FS, speechlike, through_rate, to_int16, ulaw_decode

KEY = W.Watermark(0x0123456789ABCDEF)
OTHER = W.Watermark(0xFEDCBA9876543210)
SEEDS = range(12)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- tables
def test_chip_table_is_pinned_and_balanced():
    c = W.chips(KEY.key)
    assert c.shape == (W.PERIOD,) and W.PERIOD == 15360 and set(np.unique(c)) == {-1.0, 1.0}
    # splitmix64 by hand for the first chips of this key (python integers, wrapping at 64 bits)
    m = (1 << 64) - 1
    for i in (0, 1, 2, 3, 479, 480, 15359):
        z = (KEY.key ^ (i * 0xD1342543DE82EF95 & m)) & m
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        assert c[i] == (1.0 if z >> 63 else -1.0), i
    assert [int(v) for v in W.chips(0)[:16]] == [1, 1, -1, -1, -1, -1, 1, 1, 1, -1, -1, -1, 1, 1, 1, -1]
    # balance: |sum| of 15360 fair signs stays within 4 sigma = 4 sqrt(15360) (probability of a miss 6e-5 per key)
    for k in (KEY.key, OTHER.key, 0, 1, (1 << 64) - 1):
        assert abs(W.chips(k).sum()) <= 4.0 * np.sqrt(W.PERIOD), k
    assert np.mean(W.chips(KEY.key) == W.chips(OTHER.key)) < 0.52 and np.mean(W.chips(0) == W.chips(1)) < 0.52


def test_shaping_filter_is_pinned():
    h = W.shaping_filter()
    assert h.shape == (65,) and h.dtype == np.float64
    assert abs(np.sum(h * h) - 1.0) <= 1e-15
    assert np.allclose(h, h[::-1], rtol=0, atol=1e-17)  # linear phase: the matched filter is h itself
    assert abs(h[32] - 0.5183714854454) < 1e-12 and abs(h[31] - 0.4405147118960327) < 1e-12 and abs(h[0] - 0.0011233508756799948) < 1e-12
    import math  # the definition again, tap by tap in python floats

    def lp(fc, k):
        t = 2.0 * fc / 24000.0 * (k - 32)
        return 2.0 * fc / 24000.0 * (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t))

    g = [(lp(3400.0, k) - lp(500.0, k)) * (0.54 - 0.46 * math.cos(2.0 * math.pi * k / 64)) for k in range(65)]
    e = math.sqrt(sum(v * v for v in g))
    assert max(abs(g[k] / e - h[k]) for k in range(65)) <= 1e-15
    # 5 Hz bins.  A 65-tap Hamming design has a transition band of 3.3 * 24000 / 65 = 1.2 kHz, wider than the 500 Hz edge is
    # from DC: flat at 1-3 kHz, 20 dB down at DC, and gone (34 dB) from 5 kHz up, 1.2 kHz past the upper edge
    f = np.abs(np.fft.rfft(h, 4800))
    assert f[200:600].min() > 0.7 * f.max() and f[0] < 0.1 * f.max() and f[1000:].max() < 0.02 * f.max()


def test_keys_and_strengths_are_checked():
    assert W.check_key("00ff") == 255 and W.check_key("0123456789abcdef") == KEY.key and W.check_key(7) == 7
    for bad in ("", "xyz", "0" * 17, -1, 1 << 64, 1.5, True, None):
        with pytest.raises(ValueError, match="key"):
            W.check_key(bad)
    for bad in (-40.5, -19.9, 0, float("nan"), "loud", True):
        with pytest.raises(ValueError, match="strength"):
            W.Watermark(1, bad)
    assert W.Watermark(1).strength_db == -26.0 and abs(W.Watermark(1, -20).gain - 0.1) < 1e-15
    assert "0123456789" not in repr(KEY).lower() and str(KEY.key) not in repr(KEY)  # the key stays out of logs
    assert KEY.packed().size == 65 + 15360


# ------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def marked():
    """{seed: (signal, marked signal)} of the 2 s speech-like signals at -26 dB, computed once."""
    return {s: (x, W.embed(x, KEY)) for s in SEEDS for x in [speechlike(s, 2.0)]}


@pytest.mark.parametrize("cut", [1, 479, 480, 481, 1920, 7680])
def test_output_does_not_depend_on_the_cuts(marked, cut):
    x, whole = marked[3]
    n = x.size if cut > 1 else 2500  # (sample by sample over the first blocks only: the model is a python loop)
    st = W.StreamState(KEY)
    got = np.concatenate([st.process(x[i:i + cut]) for i in range(0, n, cut)])
    assert np.array_equal(_bits(got), _bits(whole[:n]))
    ref = W.StreamState(KEY)
    ref.process(x[:n])
    assert st.state()["pos"] == n and np.array_equal(st.state()["values"].view(np.uint64), ref.state()["values"].view(np.uint64))
    assert st.process(x[:0]).size == 0


def test_mixed_cuts_and_the_whole(marked):
    x, whole = marked[5]
    rng = np.random.default_rng(2)
    st, i, got = W.StreamState(KEY), 0, []
    while i < x.size:
        n = int(rng.choice([0, 1, 7, 16, 479, 480, 481, 1920, 7680]))
        got.append(st.process(x[i:i + n]))
        i += n
    assert np.array_equal(_bits(np.concatenate(got)), _bits(whole))


def test_gain_zero_silence_and_block_zero(marked):
    x, y = marked[0]
    assert np.array_equal(_bits(W.StreamState(KEY, gain=0.0).process(x)), _bits(x))  # gain 0: the input's bits
    assert np.array_equal(_bits(y[:W.L]), _bits(x[:W.L])) and not np.array_equal(y[W.L:2 * W.L], x[W.L:2 * W.L])  # g_0 = 0
    z = np.zeros(5000, np.float32)
    assert np.array_equal(_bits(W.embed(z, KEY)), _bits(z))
    # the mark outlives a speech offset by one block, at the previous block's level, and no longer (plus the filter's 64 taps)
    burst = np.concatenate([x[:4800], np.zeros(4800, np.float32)])
    w = W.embed(burst, KEY) - burst
    assert np.any(w[4800:5280] != 0) and not np.any(w[5280 + 64:])


def test_signal_to_mark_ratio_is_the_strength():
    rng = np.random.default_rng(9)
    x = (0.1 * rng.standard_normal(4 * FS)).astype(np.float32)
    for db in (-26.0, -40.0, -20.0):
        w = W.embed(x, W.Watermark(KEY.key, db)).astype(np.float64) - x
        smr = 10.0 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum(w ** 2))
        print(f"strength {db:g} dB: signal-to-mark ratio {smr:.2f} dB")
        assert abs(smr + db) <= 0.5


# ------------------------------------------------------------------------------- detection
def _flac_round_trip(y):
    enc = flac.StreamEncoder(24000)
    s16 = flac.quantize(y)
    data = flac.stream_header(24000) + b"".join(enc.feed(s16[i:i + 1920], last=i + 1920 >= s16.size) for i in range(0, s16.size, 1920))
    return np.asarray(decode_mono16(data), np.int16)


CHANNELS = {
    "as is": lambda y: (y, FS),
    "int16": lambda y: (to_int16(y), FS),
    "crop 3217": lambda y: (y[3217:], FS),
    "pcm_8000": lambda y: (through_rate(y, 8000), 8000),
    "ulaw_8000": lambda y: (ulaw_decode(lin2ulaw(through_rate(y, 8000))), 8000),
    "pcm_16000": lambda y: (through_rate(y, 16000), 16000),
    "pcm_22050": lambda y: (through_rate(y, 22050), 22050),
    "pcm_44100": lambda y: (through_rate(y, 44100), 44100),
    "pcm_48000": lambda y: (through_rate(y, 48000), 48000),
    "flac": lambda y: (_flac_round_trip(y), FS),
    "gain 0.3": lambda y: (0.3 * y, FS),
}


@pytest.mark.parametrize("channel", sorted(CHANNELS))
def test_marked_signals_are_detected_through_every_channel(marked, channel):
    scores = []
    for s in SEEDS:
        pcm, rate = CHANNELS[channel](marked[s][1])
        d = W.detect(pcm, KEY.key, rate)
        scores.append(d.score)
        assert d.detected, (channel, s, d)
        assert (d.offset == 0) if channel != "crop 3217" else (d.offset == 3217), (channel, s, d)
    print(f"{channel}: scores {min(scores):.2f} .. {max(scores):.2f}")


def test_flac_round_trip_is_the_quantised_signal(marked):
    y = marked[1][1]
    assert np.array_equal(_flac_round_trip(y), flac.quantize(y))


def test_unmarked_wrong_key_noise_sine_and_silence_are_not_detected(marked):
    scores = []
    for s in SEEDS:
        x, y = marked[s]
        for what, pcm, key in (("unmarked", x, KEY.key), ("other key", y, OTHER.key), ("other key's mark", W.embed(x, OTHER), KEY.key)):
            d = W.detect(pcm, key)
            scores.append(d.score)
            assert not d.detected and np.isfinite(d.score), (what, s, d)
    rng = np.random.default_rng(4)
    noise = W.detect(rng.standard_normal(2 * FS) * 0.1, KEY.key)
    sine = W.detect(np.sin(2.0 * np.pi * 997.0 * np.arange(2 * FS) / FS), KEY.key)
    scores += [noise.score, sine.score]
    assert not noise.detected and not sine.detected
    print(f"negatives: largest score {max(scores):.2f}")
    for silent in (np.zeros(2 * FS), np.zeros(100), np.zeros(0), np.zeros(2 * FS, np.int16), np.full(3, 0.5)):
        d = W.detect(silent, KEY.key)
        assert d.score == 0.0 and not d.detected and isinstance(d.score, float)
    got = W.detect(marked[2][1], [OTHER.key, "0123456789abcdef", 5])  # candidates: one detection per key
    assert [d.detected for d in got] == [False, True, False]


def test_command_line_detects_a_wav_file(tmp_path, marked, capsys):
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    x, y = marked[4]
    (tmp_path / "y.wav").write_bytes(pcm_to_wav_bytes(y, 24000))
    (tmp_path / "x.wav").write_bytes(pcm_to_wav_bytes(x, 24000))
    assert W.main(["detect", str(tmp_path / "y.wav"), "--key", "0123456789abcdef"]) == 0
    assert "detected=true" in capsys.readouterr().out
    assert W.main(["detect", str(tmp_path / "x.wav"), "--key", "0123456789abcdef"]) == 1
    assert W.main(["detect", str(tmp_path / "y.wav"), "--key", "fedcba9876543210"]) == 1
    assert "detected=false" in capsys.readouterr().out


# ------------------------------------------------------------------------------- routing
FORMATS = ("pcm_24000", "pcm_16000", "ulaw_8000")
COMBOS = [(seg, q, f, fl) for seg, q, f, fl in itertools.product((False, True), (65536, 32768), FORMATS, (False, True))
          if not (fl and f.startswith("ulaw"))]


def _route(seg, q, fmt, fl, loud=None, mark=0.0):
    rate, enc = parse_stream_format(fmt)
    return engine.SlotRoute(rate, enc, q, fl, segmented=seg, loudness=loud, watermark_gain=mark)


def test_stage_names_are_unchanged():
    assert engine.STAGES == ("seam", "stretch", "resample", "flac")
    assert engine.LAUNCH_ORDER == ("seam", "loudness", "stretch", "resample", "flac")
    assert engine.PASS_ORDER == ("seam", "loudness", "stretch", "watermark", "resample", "flac")
    assert [s for s in engine.PASS_ORDER if s != "watermark"] == list(engine.LAUNCH_ORDER)


def test_marked_slots_beside_every_existing_combination():
    for c1, c2 in itertools.product(COMBOS, COMBOS):
        batch = {0: _route(*c1), 1: _route(*c2, mark=0.05), 2: engine.SlotRoute(), 3: _route(*c1, loud=-30.0, mark=0.01)}
        plan = engine.plan_pass(batch)
        assert plan.stages == [s for s in engine.PASS_ORDER if any(s in r.stages for r in batch.values())]
        i = plan.stages.index("watermark")
        assert set(plan.stages[:i]) <= {"seam", "loudness", "stretch"} and set(plan.stages[i + 1:]) <= {"resample", "flac"}
        assert plan.rows["watermark"] == [1, 3]
        for b, r in batch.items():
            assert plan.source[b] == (r.stages[-1] if r.stages else None)
            assert ("watermark" in r.stages) == (r.watermark_gain > 0)
            if r.watermark_gain > 0:  # the last float stage: only the conversion and the framing stand behind it
                assert set(r.stages[r.stages.index("watermark") + 1:]) <= {"resample", "flac"}
        # slot 0 skips the stage but a later stage reads its rows: passed through; the plain slot never is
        assert plan.through["watermark"] == ([0] if set(batch[0].stages) & {"resample", "flac"} else [])
        assert ("watermark" in plan.host) == any(r.stages and r.stages[-1] == "watermark" for r in batch.values())


def test_plans_without_a_marked_slot_are_todays():
    def todays(routes):  # plan_pass as it was before the stage existed, over LAUNCH_ORDER
        order = engine.LAUNCH_ORDER
        paths = {b: tuple(s for s, o in zip(order, (r.segmented, r.loudness is not None, r.speed_q != 65536, r.enc != 0, r.flac)) if o)
                 for b, r in routes.items()}
        rows = {s: [b for b, p in paths.items() if s in p] for s in order}
        stages = [s for s in order if rows[s]]
        through = {s: [b for b, p in paths.items() if p and s not in p and order.index(p[-1]) > order.index(s)]
                   for s in ("seam", "loudness", "stretch") if rows[s]}
        source = {b: (p[-1] if p else None) for b, p in paths.items()}
        return stages, {s: rows[s] for s in stages}, through, source, [s for s in stages if s in source.values()]

    for c1, c2, loud in itertools.product(COMBOS, COMBOS, (None, -20.0)):
        routes = {0: _route(*c1), 1: engine.SlotRoute(), 2: _route(*c2, loud=loud)}
        plan = engine.plan_pass(routes)
        assert (plan.stages, plan.rows, plan.through, plan.source, plan.host) == todays(routes)
        assert "watermark" not in plan.stages and "watermark" not in plan.rows and "watermark" not in plan.through
    assert engine.SlotRoute().watermark_gain == 0.0 and engine.SlotRoute().stages == ()
    assert engine.SlotRoute(watermark_gain=0.05).stages == ("watermark",)


def test_converter_makes_no_watermark_stage_until_a_slot_asks(monkeypatch):
    import torch

    made = []

    class Stage:
        def __init__(self, device, batch, wm):
            made.append(("watermark", wm))

        def reset_slots(self, slots, gains):
            made.append(("reset", list(slots), list(gains)))

        def close(self):
            pass

    monkeypatch.setattr(route, "Watermarker", Stage)
    conv = engine.StreamConverter(torch.device("cpu"), 4, 1920, watermark=KEY)
    conv.reset_slots([0, 1], [None, None], [None, None])
    conv.reset_slots([0, 1], [None, None], [None, None], watermark=[False, False])
    assert made == [] and not conv.converts(0) and conv.wm is None
    conv.reset_slots([1], [None], [None], watermark=[True])
    assert made == [("watermark", KEY), ("reset", [1], [KEY.gain])] and conv.converts(1) and not conv.converts(0)
    assert conv.routes[1].watermark_gain == KEY.gain and conv.ends([1]) == (False, False)
    assert conv.plan([0, 1]).stages == ["watermark"] and conv.plan([0]).stages == []
    conv.reset_slots([1], [None], [None])  # the slot's next tenant is unmarked: the stage switches it off
    assert made[-1] == ("reset", [1], [0.0]) and not conv.converts(1)
    plain = engine.StreamConverter(torch.device("cpu"), 2, 1920)
    with pytest.raises(ValueError, match="no key"):
        plain.reset_slots([0], [None], [None], watermark=[True])


# ------------------------------------------------------------------------------- requests and settings
def test_parse_request_checks_the_flag():
    assert parse_request("hi").watermark is None and parse_request("hi", watermark=None).watermark is None
    assert parse_request("hi", watermark=True).watermark is True and parse_request("hi", stream=True, watermark=False).watermark is False
    for bad in (1, 0, "yes", -26.0, KEY):
        with pytest.raises(ValueError, match="watermark"):
            parse_request("hi", watermark=bad)


def test_settings_are_parsed():
    from pydantic import ValidationError

    from smoltts_amd.server.settings import ServerSettings, watermark_setting

    assert ServerSettings(checkpoint_dir="x").watermark is None and watermark_setting(None) is None
    st = ServerSettings(checkpoint_dir="x", watermark={"key": "0123456789ABCDEF"})
    assert st.watermark.strength_db == -26.0 and st.watermark.apply == "all" and st.watermark.to_watermark() == KEY
    assert "0123456789" not in repr(st.watermark)
    st = ServerSettings(**ServerSettings(checkpoint_dir="x", watermark={"key": "00000000000000ff", "strength_db": -30, "apply": "cloned"}).model_dump())
    assert st.watermark.to_watermark() == W.Watermark(255, -30.0) and st.watermark.apply == "cloned"
    for bad in ({"key": "123"}, {"key": "0123456789abcdeg"}, {"key": "0" * 16, "strength_db": -19.0}, {"key": "0" * 16, "strength_db": -41.0},
                {"key": "0" * 16, "apply": "some"}, {"strength_db": -26.0}):
        with pytest.raises(ValidationError):
            ServerSettings(checkpoint_dir="x", watermark=bad)


# ------------------------------------------------------------------------------- HTTP
class _MarkTTS:
    """A model that marks with the numpy model when asked to, and records the keywords it is called with."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", voice, dict(kw)))
        x = speechlike(1, 2.0)
        return W.embed(x, KEY) if kw.get("watermark") else x

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", voice, dict(kw)))
        x = speechlike(1, 2.0)
        st = W.StreamState(KEY) if kw.get("watermark") else None
        for i in range(0, x.size, 1920):
            yield st.process(x[i:i + 1920]) if st is not None else x[i:i + 1920]


def _client(model, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    app = create_app(model, settings=settings)
    return TestClient(app), app.state.tts_core


SETTING = {"key": "0123456789abcdef", "strength_db": -26.0, "apply": "all"}


def test_without_the_setting_nothing_changes():
    model = _MarkTTS()
    c, core = _client(model)
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert r.status_code == 200 and "x-watermark" not in r.headers and model.calls[-1] == ("call", "sky", {})
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "hi"})
    assert r.status_code == 200 and "x-watermark" not in r.headers and model.calls[-1] == ("stream", "sky", {})
    assert c.post("/v1/watermark/detect", json={"audio": "AAAA"}).status_code == 404
    assert core.watermark is None


def test_apply_all_marks_every_route_and_detect_answers():
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    model = _MarkTTS()
    c, core = _client(model, {"watermark": SETTING})
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert r.status_code == 200 and r.headers["x-watermark"] == "1" and model.calls[-1] == ("call", "sky", {"watermark": True})
    assert r.content == pcm_to_wav_bytes(W.embed(speechlike(1, 2.0), KEY), 24000)
    d = c.post("/v1/watermark/detect", json={"audio": base64.b64encode(r.content).decode()})
    assert d.status_code == 200 and d.json()["detected"] is True and d.json()["score"] >= W.THRESHOLD and set(d.json()) == {"detected", "score"}
    plain = pcm_to_wav_bytes(speechlike(1, 2.0), 24000)
    d = c.post("/v1/watermark/detect", json={"audio": base64.b64encode(plain).decode()})
    assert d.status_code == 200 and d.json()["detected"] is False
    assert c.post("/v1/watermark/detect", json={"audio": "not base64!"}).status_code == 422
    assert c.post("/v1/watermark/detect", json={"audio": base64.b64encode(b"RIFFxxxx").decode()}).status_code == 422
    assert c.post("/v1/watermark/detect", json={}).status_code == 422
    r = c.post("/v1/text-to-speech/sky", json={"text": "hi"})
    assert r.headers["x-watermark"] == "1" and model.calls[-1] == ("call", "sky", {"watermark": True})
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "hi"})
    assert r.status_code == 200 and r.headers["x-watermark"] == "1" and model.calls[-1] == ("stream", "sky", {"watermark": True})
    assert W.detect(np.frombuffer(r.content, np.float32), KEY.key).detected
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "response_format": "pcm"})
    assert r.status_code == 200 and r.headers["x-watermark"] == "1" and W.detect(np.frombuffer(r.content, "<i2"), KEY.key).detected
    for resp in (r, d):  # the key is never returned
        assert "0123456789abcdef" not in resp.text.lower() and not any("0123456789abcdef" in v.lower() for v in resp.headers.values())


def test_apply_cloned_marks_registered_voices_only():
    model = _MarkTTS()
    c, core = _client(model, {"watermark": dict(SETTING, apply="cloned")})
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert r.status_code == 200 and "x-watermark" not in r.headers and model.calls[-1] == ("call", "sky", {"watermark": False})
    core.voices["cv_0123"] = {"name": "mine", "prompt_positions": 10}  # (as POST /v1/voices/add leaves it)
    r = c.post("/v1/text-to-speech/cv_0123", json={"text": "hi"})
    assert r.status_code == 200 and r.headers["x-watermark"] == "1" and model.calls[-1] == ("call", "cv_0123", {"watermark": True})
    r = c.post("/v1/text-to-speech/cv_0123/stream", json={"text": "hi"})
    assert r.headers["x-watermark"] == "1" and model.calls[-1] == ("stream", "cv_0123", {"watermark": True})
    r = c.post("/v1/text-to-speech/nova/stream", json={"text": "hi"})
    assert "x-watermark" not in r.headers and model.calls[-1] == ("stream", "nova", {"watermark": False})
