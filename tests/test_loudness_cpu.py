"""Loudness normalisation, host side (no GPU): the numpy model ``smoltts_amd/loudness.py`` against an independent BS.1770-4 meter
written here with scipy, the blocking and the stream rule, the stage's place in ``engine.plan_pass``, and the request and HTTP
checks."""
import itertools

import numpy as np
import pytest
from scipy.signal import lfilter

from smoltts_amd import engine, loudness as L, route
from smoltts_amd.formats import parse_stream_format
from smoltts_amd.request import parse_request

FS = L.FS


# ------------------------------------------------------------------------------- signals
def _sine(seconds, amp, f=997.0):
    return (amp * np.sin(2 * np.pi * f * np.arange(int(seconds * FS)) / FS)).astype(np.float32)


def _noise(seed, seconds, amp):
    x = np.random.default_rng(seed).standard_normal(int(seconds * FS))
    return (amp * np.convolve(x, np.ones(8) / 8, mode="same")).astype(np.float32)


def _bursts(seed, seconds, amp):
    x = _noise(seed, seconds, amp)
    t = np.arange(x.size) / FS
    return (x * (np.sin(2 * np.pi * 0.8 * t) > -0.2)).astype(np.float32)


def _loud_then_quiet(seed):
    return np.concatenate([_noise(seed, 3.0, 0.3), _noise(seed + 1, 3.0, 0.3 * 10 ** (-25 / 20))])


def _reference_meter(x, fs=FS):
    """BS.1770-4 for mono, written independently of the model: scipy's lfilter, plain numpy gating.  -> (LUFS, blocks, blocks past
    the absolute gate, blocks past both)."""
    sb, sa, hb, ha = L.k_weighting(fs)
    y = lfilter(hb, ha, lfilter(sb, sa, np.asarray(x, np.float64)))
    hop = fs // 10
    nb = x.size // hop - 3
    z = np.array([np.mean(y[j * hop:(j + 4) * hop] ** 2) for j in range(max(nb, 0))])
    lk = -0.691 + 10 * np.log10(np.maximum(z, 1e-300))
    a = lk > -70.0
    if not a.any():
        return float("-inf"), z.size, 0, 0
    rel = -0.691 + 10 * np.log10(z[a].mean()) - 10.0
    b = a & (lk > rel)
    return float(-0.691 + 10 * np.log10(z[b].mean())), z.size, int(a.sum()), int(b.sum())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- coefficients
def test_coefficient_formula_gives_the_standards_48k_table():
    sb, sa, hb, ha = L.k_weighting(48000)
    assert np.allclose(sb, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-12)
    assert np.allclose(sa, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-12)
    assert np.array_equal(hb, [1.0, -2.0, 1.0])
    assert np.allclose(ha, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-12)


def test_coefficients_at_24k_and_the_sine_reading():
    sb, sa, hb, ha = L.k_weighting()
    assert np.allclose(sb, [1.48790022, -2.24620547, 0.90490912], atol=5e-9) and np.allclose(sa[1:], [-1.39023461, 0.53683848], atol=5e-9)
    assert np.allclose(ha[1:], [-1.98014413, 0.98024282], atol=5e-9)
    assert abs(L.measure(_sine(5.0, 1.0))[0] - (-2.98)) < 0.005
    assert abs(_reference_meter(_sine(5.0, 1.0, ), 24000)[0] - (-2.98)) < 0.005
    x48 = np.sin(2 * np.pi * 997.0 * np.arange(5 * 48000) / 48000)
    assert abs(_reference_meter(x48, 48000)[0] - (-3.01)) < 0.005  # the 0.03 LU is the bilinear warping at 24 kHz


# ------------------------------------------------------------------------------- the meter
@pytest.mark.parametrize("name, x", [("sine", _sine(5.0, 0.25)), ("bursts", _bursts(1, 8.0, 0.1)), ("loud-quiet", _loud_then_quiet(2)),
                                     ("long", _bursts(3, 140.0, 0.05))], ids=lambda v: v if isinstance(v, str) else "")
def test_meter_equals_an_independent_one(name, x):
    lufs, peak = L.measure(x)
    ref, nb, n1, n2 = _reference_meter(x)
    print(f"{name}: model {lufs:.9f} LUFS, reference {ref:.9f}, blocks {nb} / {n1} / {n2}")
    assert abs(lufs - ref) <= 1e-6
    assert peak == float(np.abs(x).max())
    if name == "loud-quiet":
        assert n2 < n1 <= nb, "the relative gate must drop blocks of this signal"
    hops, _ = L.hop_energies(x)
    z = np.array([L._block(*hops[j:j + 4]) for j in range(hops.size - 3)])
    assert L.gated_power(z)[1:] == (n1, n2)


def test_meter_of_nothing():
    assert L.measure(np.zeros(FS, np.float32)) == (float("-inf"), 0.0)
    assert L.measure(_sine(0.39, 0.5))[0] == float("-inf")
    assert L.measure(np.zeros(0, np.float32)) == (float("-inf"), 0.0)


# ------------------------------------------------------------------------------- the blocking rule
def test_blocking_rule_reaches_the_target_or_the_ceiling():
    x = _bursts(4, 6.0, 0.05)
    y, g = L.normalize(x, -20.0)
    assert g * np.abs(x).max() < L.tables().ceiling  # the cap is idle
    assert abs(L.measure(y)[0] - (-20.0)) <= 1e-6 and abs(_reference_meter(y)[0] - (-20.0)) <= 1e-6
    x = _bursts(4, 6.0, 0.05)
    x[30000] = 0.9  # one tall sample: the gain to -8 LUFS would clip it
    y, g = L.normalize(x, -8.0)
    assert np.abs(y).max() == np.float32(L.tables().ceiling) and L.measure(y)[0] < -8.0
    assert g == L.tables().ceiling / np.float64(np.float32(0.9))


def test_blocking_rule_leaves_silence_and_short_inputs_alone():
    for x in (np.zeros(2 * FS, np.float32), _sine(0.3, 0.1), np.zeros(0, np.float32)):
        y, g = L.normalize(x, -16.0)
        assert g == 1.0 and np.array_equal(_bits(y), _bits(x))


# ------------------------------------------------------------------------------- the stream rule
def test_stream_rule_does_not_depend_on_how_calls_cut_the_stream():
    x = np.concatenate([_bursts(5, 1.5, 0.02), _noise(6, 0.7, 0.2)])
    whole = L.StreamState(-18.0, 3.0)
    want = whole.process(x)
    assert want.size == x.size and whole.knots[-1] != whole.knots[0]
    for step in (1, 1920, 7680):
        s = L.StreamState(-18.0, 3.0)
        got = np.concatenate([s.process(x[i:i + step]) for i in range(0, x.size, step)])
        assert got.tobytes() == want.tobytes(), step
        a, b = s.state(), whole.state()
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_knots_obey_the_slew_and_wait_for_the_gate():
    lead = int(1.3 * FS)
    x = np.concatenate([np.zeros(lead, np.float32), _noise(7, 6.0, 0.01), _noise(8, 3.0, 0.5)])
    s = L.StreamState(-20.0)
    s.process(x)
    k = np.asarray(s.knots)
    passed = np.asarray(s.passed)
    assert k.size == x.size // L.HOP + 2 and np.abs(k).max() <= L.K_MAX
    up = np.diff(k)
    assert up.max() <= L.SLEW_STEPS and up.max() > 0
    # a knot falls faster than the slew only onto the running peak's cap (the loud part arrives at +20 dB of gain)
    caps = np.asarray(s.caps)
    fast = up < -L.SLEW_STEPS
    assert fast.sum() >= 1 and np.all(k[1:][fast] == caps[1:][fast]) and np.all(k <= caps)
    assert (up == -L.SLEW_STEPS).sum() > 5
    assert np.all(k[passed == 0] == k[0]) and (passed == 0).sum() == lead // L.HOP + 2  # the first block with noise in it passes
    assert np.all(k[: lead // L.HOP + 2] == 0)
    # both knots of hop h were fixed from the samples in front of it: the same knots with everything from hop h on replaced
    h = 40
    t = L.StreamState(-20.0)
    t.process(np.concatenate([x[: h * L.HOP], np.ones(5 * L.HOP, np.float32)]))
    assert t.knots[: h + 2] == s.knots[: h + 2]


def test_peak_cap_holds_a_knot_down():
    x = _noise(9, 4.0, 0.004)
    x[100] = 0.5
    s = L.StreamState(-10.0, 0.0)
    y = s.process(x)
    cap = 20 * np.log10(L.tables().ceiling / 0.5)
    assert max(s.knots) == int(np.floor(cap * L.GRID)) and np.abs(y).max() <= L.tables().ceiling


STEADY_LU = 0.01  # measured with this model on the two signals below: 0.0094 and 0.0074 LU


@pytest.mark.parametrize("x", [_sine(10.0, 0.05), _noise(5, 10.0, 0.02)], ids=["sine", "noise"])
def test_stream_rule_settles_at_the_target(x):
    l0 = L.measure(x)[0]
    target = l0 + 12.0
    y = L.StreamState(target).process(x)
    settled = int((12.0 / 5.0 + 0.4) * FS)
    err = L.measure(y[settled:])[0] - target
    print(f"input {l0:.3f} LUFS, target {target:.3f}, settled error {err:+.5f} LU")
    assert abs(err) <= STEADY_LU + 1.0 / L.GRID


# ------------------------------------------------------------------------------- routing
FORMATS = ("pcm_24000", "pcm_16000", "ulaw_8000")
COMBOS = [(seg, q, f, fl) for seg, q, f, fl in itertools.product((False, True), (65536, 32768), FORMATS, (False, True))
          if not (fl and f.startswith("ulaw"))]


def _route(seg, q, fmt, fl, loud=None):
    rate, enc = parse_stream_format(fmt)
    return engine.SlotRoute(rate, enc, q, fl, segmented=seg, loudness=loud)


def test_stage_names():
    assert engine.STAGES == ("seam", "stretch", "resample", "flac")
    assert engine.LAUNCH_ORDER == ("seam", "loudness", "stretch", "resample", "flac")


def test_loudness_slots_beside_every_existing_combination():
    for c1, c2 in itertools.product(COMBOS, COMBOS):
        batch = {0: _route(*c1), 1: _route(*c2, loud=-20.0), 2: engine.SlotRoute(), 3: _route(*c1, loud=-30.0)}
        plan = engine.plan_pass(batch)
        assert plan.stages == [s for s in engine.LAUNCH_ORDER if any(s in r.stages for r in batch.values())]
        i = plan.stages.index("loudness")
        assert plan.stages[:i] in ([], ["seam"]) and "seam" not in plan.stages[i:]
        assert plan.rows["loudness"] == [1, 3]
        for b, r in batch.items():
            assert plan.source[b] == (r.stages[-1] if r.stages else None)
            want = ("seam",) * r.segmented + ("loudness",) * (r.loudness is not None)
            assert r.stages[:len(want)] == want
        # slot 0 skips the stage but a later stage reads its rows: passed through; the plain slot never is
        assert plan.through["loudness"] == ([0] if set(batch[0].stages) - {"seam"} else [])
        assert ("loudness" in plan.host) == any(r.stages and r.stages[-1] == "loudness" for r in batch.values())


def test_plans_without_loudness_are_todays():
    for c1, c2 in itertools.product(COMBOS, COMBOS):
        plan = engine.plan_pass({0: _route(*c1), 1: engine.SlotRoute(), 2: _route(*c2)})
        assert "loudness" not in plan.stages and "loudness" not in plan.rows and "loudness" not in plan.through
        assert all(s in engine.STAGES for s in plan.stages) and set(plan.through) <= {"seam", "stretch"}
    assert engine.SlotRoute(24000, 0, 65536, False, segmented=True).stages == ("seam",)


def test_converter_makes_no_loudness_stage_until_a_slot_asks(monkeypatch):
    made = []

    class Stage:
        def __init__(self, *a):
            made.append("loudness")

        def reset_slots(self, *a):
            made.append("reset")

        def close(self):
            pass

    monkeypatch.setattr(route, "LoudnessNormalizer", Stage)
    conv = engine.StreamConverter(torch_device(), 4, 1920)
    conv.reset_slots([0, 1], [None, None], [None, None])
    assert made == [] and not conv.converts(0)
    conv.reset_slots([1], [None], [None], None, [-20.0], [1.5])
    assert made == ["loudness", "reset"] and conv.converts(1) and not conv.converts(0)
    assert conv.routes[1].loudness == -20.0 and conv.routes[1].start_gain_db == 1.5 and conv.ends([1]) == (False, False)
    assert conv.plan([0, 1]).stages == ["loudness"] and conv.plan([0]).stages == []


def torch_device():
    import torch

    return torch.device("cpu")


# ------------------------------------------------------------------------------- requests
def test_parse_request_checks_the_target():
    assert parse_request("hi").loudness is None and parse_request("hi", loudness=None).loudness is None
    assert parse_request("hi", loudness=-23).loudness == -23.0 and parse_request("hi", loudness=-5.0).loudness == -5.0
    assert parse_request("hi", stream=True, loudness=-40.0, loudness_start_gain_db=6).start_gain_db == 6.0
    for bad in (-40.01, -4.99, 0.0, float("nan"), float("inf"), "loud", True):
        with pytest.raises(ValueError, match="loudness"):
            parse_request("hi", loudness=bad)
    with pytest.raises(ValueError, match="start_gain"):
        parse_request("hi", stream=True, loudness=-20.0, loudness_start_gain_db=21.0)
    with pytest.raises(ValueError, match="start_gain"):
        parse_request("hi", stream=True, loudness_start_gain_db=1.0)  # no target
    with pytest.raises(ValueError, match="start_gain"):
        parse_request("hi", loudness=-20.0, loudness_start_gain_db=1.0)  # not a stream


class _LoudTTS:
    """A model that levels with the numpy model, and records the keywords it is called with."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []
        self.last_loudness_gain_db = None

    def __call__(self, text, voice="heart", **kw):
        self.calls.append(("call", dict(kw)))
        x = _bursts(1, 3.0, 0.05)
        if "loudness" in kw:
            x, g = L.normalize(x, kw["loudness"])
            self.last_loudness_gain_db = L.gain_db(g)
        return x

    def stream(self, text, voice="heart", **kw):
        self.calls.append(("stream", dict(kw)))
        x = _bursts(1, 3.0, 0.05)
        st = L.StreamState(kw["loudness"], kw.get("loudness_start_gain_db", 0.0)) if "loudness" in kw else None
        for i in range(0, x.size, 1920):
            yield st.process(x[i:i + 1920]) if st is not None else x[i:i + 1920]


def _client(model, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    return TestClient(create_app(model, settings=settings))


def test_http_loudness_field_and_header():
    model = _LoudTTS()
    c = _client(model)
    plain = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert plain.status_code == 200 and "x-loudness-gain-db" not in plain.headers and model.calls[-1] == ("call", {})
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "loudness": -20})
    assert r.status_code == 200 and model.calls[-1] == ("call", {"loudness": -20.0})
    want, g = L.normalize(_bursts(1, 3.0, 0.05), -20.0)
    assert r.headers["x-loudness-gain-db"] == f"{L.gain_db(g):.2f}"
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    assert r.content == pcm_to_wav_bytes(want, 24000) and r.content != plain.content
    off = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "loudness": None})
    assert off.status_code == 200 and off.content == plain.content and model.calls[-1] == ("call", {})
    r = c.post("/v1/text-to-speech/sky", json={"text": "hi", "loudness": -16.5})
    assert r.status_code == 200 and "x-loudness-gain-db" in r.headers and model.calls[-1] == ("call", {"loudness": -16.5})
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "hi", "loudness": -16.5, "loudness_start_gain_db": 3})
    assert r.status_code == 200 and model.calls[-1] == ("stream", {"loudness": -16.5, "loudness_start_gain_db": 3.0})
    assert r.content == L.stream_normalize(_bursts(1, 3.0, 0.05), -16.5, 3.0).tobytes()
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "response_format": "pcm", "loudness": -30})
    assert r.status_code == 200 and model.calls[-1] == ("stream", {"loudness": -30.0})


@pytest.mark.parametrize("bad", [-40.5, -4.0, 0, 3.0])
def test_http_answers_400_outside_the_range(bad):
    model = _LoudTTS()
    c = _client(model)
    for path, body in (("/v1/audio/speech", {"input": "hi", "voice": "sky"}), ("/v1/text-to-speech/sky", {"text": "hi"}),
                       ("/v1/text-to-speech/sky/stream", {"text": "hi"}),
                       ("/v1/audio/speech", {"input": "hi", "voice": "sky", "response_format": "flac"})):
        r = c.post(path, json=dict(body, loudness=bad))
        assert r.status_code == 400 and "loudness" in r.json()["detail"], (path, r.status_code)
    assert model.calls == []


def test_server_setting_is_the_default_and_null_switches_it_off():
    model = _LoudTTS()
    c = _client(model, settings={"loudness": -23.0})
    assert c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"}).status_code == 200
    assert model.calls[-1] == ("call", {"loudness": -23.0})
    c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "loudness": -18})
    assert model.calls[-1] == ("call", {"loudness": -18.0})
    c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "loudness": None})
    assert model.calls[-1] == ("call", {})
    c.post("/v1/text-to-speech/sky/stream", json={"text": "hi"})
    assert model.calls[-1] == ("stream", {"loudness": -23.0})
