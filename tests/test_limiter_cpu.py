"""The peak limiter's numpy model (``smoltts_amd/limiter.py``, the definition the kernel is held to in test_limiter_gpu.py): its
four properties on speech-like signals and on an isolated impulse, the stream rule over every kind of cut, the option's parse,
its way through the routing plan, the HTTP bodies and the server setting, the uncapped loudness gain, and the C exports."""
import dataclasses
import itertools
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from smoltts_amd import abi, limiter as LM, loudness, route
from smoltts_amd.formats import parse_stream_format
from smoltts_amd.request import parse_request

from limiter_helpers import CEILINGS_DB, DRIVES_DB, SEEDS, bits, driven, impulse, peak_8x, stream

ROOT = Path(__file__).resolve().parents[1]


@lru_cache(maxsize=None)
def _limited(seed: int, drive_db: float, ceiling_db: float):
    """(x, p, g, y) of one of the shared signals: computed once, read by every test."""
    x = driven(seed, drive_db)
    xd = x.astype(np.float64)
    p = LM.peaks(np.concatenate([np.zeros(5), xd, np.zeros(6)]), x.size)
    g = LM.gains(x, ceiling_db)
    y, gmin = LM.limit(x, ceiling_db)
    assert gmin == g.min()
    for a in (x, p, g, y):
        a.setflags(write=False)
    return x, p, g, y


def _quiet(p: np.ndarray, c: float) -> np.ndarray:
    """Where no p within the window of g[n] (n - 1320 .. n + 120) passes c."""
    over = np.concatenate([np.zeros(LM.R + LM.L), (p > c).astype(np.int64), np.zeros(LM.L, np.int64)])
    cs = np.concatenate([[0], np.cumsum(over)])
    w = LM.R + 2 * LM.L + 1
    return cs[w:] - cs[:-w] == 0


# ------------------------------------------------------------------------------- the model
def test_constants_and_interpolator():
    assert (LM.L, LM.R, LM.HOLD_BACK, LM.WINDOW, LM.MEAN, LM.R_HIST, LM.REACH_BACK) == (120, 1200, 126, 1321, 121, 1440, 1325)
    h = LM.interpolator()
    assert h.shape == (3, 12) and LM.packed().shape == (36,) and np.array_equal(LM.packed(), h.reshape(-1))
    assert np.allclose(h.sum(axis=1), 1.0, atol=1e-15)
    k = np.arange(-5, 7)
    for q in (1, 2, 3):
        t = k - q / 4.0
        w = np.sinc(t) * (0.5 + 0.5 * np.cos(np.pi * t / 6.0))
        assert np.array_equal(h[q - 1], w / w.sum())
    assert np.array_equal(h[0], h[2][::-1]) or np.allclose(h[0], h[2][::-1], atol=1e-16)  # phases 1/4 and 3/4 mirror each other
    # a constant comes through every phase as itself, a sampled sine at 3 kHz within the window's error
    n = np.arange(400)
    s = np.sin(2 * np.pi * 3000.0 / 24000.0 * n)
    for q in (1, 2, 3):
        y = np.array([np.dot(h[q - 1], s[i - 5: i + 7]) for i in range(10, 390)])
        assert np.abs(y - np.sin(2 * np.pi * 3000.0 / 24000.0 * (np.arange(10, 390) + q / 4.0))).max() < 5e-3


@pytest.mark.parametrize("ceiling_db", CEILINGS_DB)
@pytest.mark.parametrize("drive_db", DRIVES_DB)
def test_properties_one_and_two_on_speech(drive_db, ceiling_db):
    c = LM.ceiling_of_db(ceiling_db)
    for seed in SEEDS:
        x, p, g, y = _limited(seed, drive_db, ceiling_db)
        assert y.dtype == np.float32 and y.shape == x.shape and g.max() <= 1.0 and g.min() > 0.0
        quiet = _quiet(p, c)
        assert np.all(g[quiet] == 1.0) and np.array_equal(bits(y[quiet]), bits(x[quiet])), (seed, drive_db, ceiling_db)
        assert np.all(g * p <= c * (1.0 + 2.0 ** -52)), (seed, float((g * p).max()), c)
        assert np.all(np.abs(y.astype(np.float64)) <= c * (1.0 + 2.0 ** -23)), (seed, float(np.abs(y).max()), c)
        if drive_db == 0.0 and ceiling_db >= -1.0:  # as they are, none passes the ceiling: the bytes leave unchanged
            assert quiet.all() and np.array_equal(bits(y), bits(x)), seed
        assert (g.min() < 1.0) == bool((p > c).any()), seed  # it engages exactly where an estimate passes the ceiling


def test_negative_zero_and_silence_leave_unchanged():
    x = np.zeros(5000, np.float32)
    x[::3] = -0.0
    x[100] = 0.25
    y, g = LM.limit(x, -6.0)
    assert g == 1.0 and np.array_equal(bits(y), bits(x))
    assert LM.limit(np.zeros(0, np.float32), -1.0)[0].size == 0 and LM.limit(np.zeros(0, np.float32), -1.0)[1] == 1.0


def test_property_three_the_output_is_a_function_of_its_window():
    x = driven(4, 12.0)[6000:18000].copy()
    y, _ = LM.limit(x, -6.0)
    rng = np.random.default_rng(9)
    for n in (1325, 4000, 7777, x.size - 127):
        x2 = x.copy()
        x2[:n - LM.REACH_BACK] = rng.uniform(-3, 3, n - LM.REACH_BACK).astype(np.float32)
        x2[n + LM.HOLD_BACK + 1:] = rng.uniform(-3, 3, x.size - n - LM.HOLD_BACK - 1).astype(np.float32)
        y2, _ = LM.limit(x2, -6.0)
        assert bits(y2[n: n + 1]) == bits(y[n: n + 1]), n
    # ... and of no less: the sample at the far end of the look-ahead counts
    x2 = x.copy()
    at = int(np.argmax(np.abs(x[2000:10000]))) + 2000
    x2[at] = 0.0
    assert not np.array_equal(LM.limit(x2, -6.0)[0][at - LM.HOLD_BACK: at], y[at - LM.HOLD_BACK: at])


@pytest.mark.parametrize("ceiling_db", CEILINGS_DB)
def test_property_four_around_an_isolated_peak(ceiling_db):
    n0 = 3000
    x = impulse(6000, n0, 2.0)
    g = LM.gains(x, ceiling_db)
    c = LM.ceiling_of_db(ceiling_db)
    lo = float(g.min())
    assert lo <= c / 2.0 * (1.0 + 2.0 ** -52) and lo > c / 2.0 * 0.7  # (the 4x estimate of one sample is at most its height ... its side lobes)
    assert np.all(np.diff(g[n0 - 2 * LM.L: n0 + 1]) <= 0.0)  # into the peak
    # flat: the mean of 121 equal minima is that minimum up to its 121 additions' and its division's roundings, 2^-53 each
    flat = np.flatnonzero(np.abs(g[n0:] - lo) <= 2.0 * 122.0 * 2.0 ** -53 * lo)
    assert flat[0] <= 6 and np.all(np.diff(flat[:LM.R - 12]) == 1) and flat.size >= LM.R - 12  # the hold
    end = n0 + int(flat[-1])
    assert np.all(np.diff(g[end: end + LM.L + 1]) >= 0.0) and np.all(np.diff(g[end:]) >= 0.0)  # the release ramp
    assert np.all(g[:n0 - 2 * LM.L] == 1.0) and np.all(g[n0 + LM.R + 2 * LM.L + 1:] == 1.0)
    y, gmin = LM.limit(x, ceiling_db)
    assert gmin == lo and abs(float(y[n0])) <= c * (1.0 + 2.0 ** -23)


# ------------------------------------------------------------------------------- the stream rule
def _check_cuts(x, db, cuts, last_empty=False):
    want, gmin = LM.limit(x, db)
    got, sizes, st = stream(x, db, cuts, last_empty)
    fed = np.minimum(np.cumsum(cuts), x.size) if len(cuts) else np.zeros(0, np.int64)
    for i, f in enumerate(fed):  # every call emits what became final: max(0, fed - 126) in total
        assert sum(sizes[: i + 1]) == max(0, int(f) - LM.HOLD_BACK), (i, int(f))
    assert got.size == x.size and np.array_equal(bits(got), bits(want))
    assert float(st.min_g) == gmin and st.ended and st.pos == x.size
    assert st.process(x[:10]).size == 0  # an ended stream takes nothing more


@pytest.mark.parametrize("chunk", [1, 7, 125, 126, 127, 1920, 7680])
def test_stream_equals_the_whole_for_every_chunk_size(chunk):
    x = driven(3, 12.0)
    hot = int(np.argmax(np.abs(x)))
    n = {1: 3000, 7: 12000}.get(chunk, x.size)  # (the small chunks over an excerpt around the largest peak: seconds, not minutes)
    lo = max(0, min(hot - n // 2, x.size - n))
    x = x[lo: lo + n]
    assert LM.limit(x, -6.0)[1] < 1.0
    _check_cuts(x, -6.0, [chunk] * (x.size // chunk))


def test_stream_equals_the_whole_for_random_cuts_empty_calls_and_an_empty_last():
    x = driven(5, 6.0)
    rng = np.random.default_rng(17)
    cuts = []
    while sum(cuts) < x.size - 4000:
        cuts.append(int(rng.choice([0, 1, 5, 126, 127, 300, 1920, 4000])))
    assert 0 in cuts
    _check_cuts(x, -1.0, cuts)
    _check_cuts(x, -1.0, cuts, last_empty=True)
    _check_cuts(x, -1.0, [0, 0, x.size], last_empty=True)
    _check_cuts(x[:100], -1.0, [50])  # shorter than the hold-back: everything leaves with `last`
    _check_cuts(x[:100], -1.0, [50, 50], last_empty=True)
    got, sizes, _ = stream(x[:0], -1.0, [])
    assert got.size == 0 and sizes == [0]


def test_model_state_is_what_the_device_keeps():
    x = driven(6, 12.0)[:9000]
    st = LM.StreamState(-6.0)
    st.process(x[:5000])
    s = st.state()
    assert s["pos"] == 5000 and s["ended"] == 0 and s["c"] == LM.ceiling_of_db(-6.0) and s["r"].shape == (1440,) and s["x"].shape == (126,)
    assert np.array_equal(s["x"], x[5000 - 126: 5000]) and s["x"].dtype == np.float32
    r = LM.required(LM.peaks(np.concatenate([np.zeros(5), x[:5006].astype(np.float64)]), 5000 - 6 + 1)[-1440:], s["c"])
    assert np.array_equal(s["r"], r)
    fresh = LM.StreamState(ceiling=0.5).state()
    assert fresh["pos"] == 0 and np.all(fresh["r"] == 1.0) and not fresh["x"].any() and fresh["min_g"] == 1.0 and fresh["c"] == 0.5


# ------------------------------------------------------------------------------- measurements (printed for DESIGN.md, not asserted)
def test_report_the_8x_reading_and_the_watermark_score(capsys):
    from smoltts_amd import watermark as W

    key = W.Watermark(0x0123456789ABCDEF, -26.0)
    with capsys.disabled():
        print("\nceiling -1 dBFS (c = %.4f): per drive, over seeds 0..11" % LM.ceiling_of_db(-1.0))
        for drive in DRIVES_DB:
            rows = [_limited(seed, drive, -1.0) for seed in SEEDS]
            share = [float(np.mean(g < 1.0)) for _, _, g, _ in rows]
            gmin = [float(g.min()) for _, _, g, _ in rows]
            own = [float((g * p).max()) for _, p, g, _ in rows]
            read = [peak_8x(y) for _, _, _, y in rows]
            print(f"  drive +{drive:g} dB: limited samples <= {100 * max(share):.1f} %, min g {min(gmin):.3f}, own estimate of the output "
                  f"<= {max(own):.4f}, 8x reading {min(read):.4f} .. {max(read):.4f}  (" + " ".join(f"{r:.3f}" for r in read) + ")")
        scores = []
        for seed in SEEDS[:4]:
            marked = W.embed(driven(seed, 6.0), key)
            scores.append((W.detect(marked, key.key).score, W.detect(LM.limit(marked, -1.0)[0], key.key).score))
        print("  watermark score, marked at +6 dB drive, unlimited -> limited at -1 dBFS: " + ", ".join(f"{a:.1f} -> {b:.1f}" for a, b in scores))


# ------------------------------------------------------------------------------- the option
def test_parse_request_checks_the_ceiling():
    assert parse_request("hi").peak_limit_db is None and parse_request("hi").ceiling == 0.0
    p = parse_request("hi", peak_limit_db=-1)
    assert p.peak_limit_db == -1.0 and isinstance(p.peak_limit_db, float) and p.ceiling == 10.0 ** (-1.0 / 20.0)
    assert parse_request("hi", peak_limit_db=0).ceiling == 1.0 and parse_request("hi", stream=True, peak_limit_db=-12.0).peak_limit_db == -12.0
    for bad, msg in ((True, "peak_limit_db must be a number of dBFS or null, not a boolean"),
                     (False, "peak_limit_db must be a number of dBFS or null, not a boolean"),
                     ("-1", "peak_limit_db must be a number of dBFS between -12 and 0, or null"),
                     ([-1.0], "peak_limit_db must be a number of dBFS between -12 and 0, or null"),
                     (float("nan"), "peak_limit_db must be a number of dBFS between -12 and 0, or null"),
                     (0.5, r"peak_limit_db 0.5 outside \[-12, 0\] dBFS"),
                     (-12.5, r"peak_limit_db -12.5 outside \[-12, 0\] dBFS")):
        with pytest.raises(ValueError, match="^" + msg + "$"):
            parse_request("hi", peak_limit_db=bad)
    # it goes with every other option: the stage copies samples one to one and only delays them
    assert parse_request("hi", peak_limit_db=-3.0, timestamps=True, speed=1.5, loudness=-20.0).timestamps
    p = parse_request("One. Two.", stream=True, output_format="pcm_16000", container="flac", segment=True, trim_silence=True,
                      max_pause_s=0.5, speed=0.8, loudness=-23.0, watermark=True, peak_limit_db=-2.0)
    assert p.ceiling == LM.ceiling_of_db(-2.0) and p.container == "flac" and p.trims
    assert LM.reduction_db(1.0) == 0.0 and LM.reduction_db(0.5) == pytest.approx(6.0206, abs=1e-4)


def test_static_gain_without_the_cap():
    target, power = -16.0, loudness.target_power(-30.0)
    free = 10.0 ** ((target - loudness.lufs_of_power(power)) / 20.0)
    assert loudness.static_gain(target, power, 0.9) == loudness.static_gain(target, power, 0.9, cap=True) == loudness.tables().ceiling / 0.9
    assert loudness.static_gain(target, power, 0.9, cap=False) == free > loudness.tables().ceiling / 0.9
    assert loudness.static_gain(target, power, 0.01, cap=False) == loudness.static_gain(target, power, 0.01) == free
    assert loudness.static_gain(target, 0.0, 0.9, cap=False) == 1.0
    x = driven(2, 0.0)
    assert loudness.normalize(x, -10.0, cap=False)[1] > loudness.normalize(x, -10.0)[1] == loudness.normalize(x, -10.0, cap=True)[1]


# ------------------------------------------------------------------------------- routing
from test_watermark_cpu import COMBOS  # noqa: E402  (the combinations every stage's routing test walks)

FLOATS = {"trim", "seam", "loudness", "stretch", "watermark"}


def _route(seg, q, fmt, fl, **kw):
    rate, enc = parse_stream_format(fmt)
    return route.SlotRoute(rate, enc, q, fl, segmented=seg, **kw)


def test_order_and_fields():
    assert route.LIMIT_ORDER == ("trim", "seam", "loudness", "stretch", "watermark", "limit", "resample", "flac")
    assert [s for s in route.LIMIT_ORDER if s != "limit"] == list(route.TRIM_ORDER)
    assert route.LIMIT_FLOAT_STAGES == route.TRIM_FLOAT_STAGES + ("limit",)
    names = [f.name for f in dataclasses.fields(route.SlotRoute)]
    assert names.index("ceiling") == names.index("watermark_gain") + 1 and names[-3:] == ["trim", "pause_blocks", "thr"]
    assert route.SlotRoute().ceiling == 0.0 and route.SlotRoute().stages == () and route.SlotRoute(ceiling=0.5).stages == ("limit",)


def test_limited_slots_beside_every_existing_combination():
    for c1, c2 in itertools.product(COMBOS, COMBOS):
        batch = {0: _route(*c1), 1: _route(*c2, ceiling=0.9), 2: route.SlotRoute(),
                 3: _route(*c1, loudness=-30.0, watermark_gain=0.01, trim=True, ceiling=0.5)}
        plan = route.plan_pass(batch)
        assert plan.stages == [s for s in route.LIMIT_ORDER if any(s in r.stages for r in batch.values())]
        i = plan.stages.index("limit")
        assert set(plan.stages[:i]) <= FLOATS and set(plan.stages[i + 1:]) <= {"resample", "flac"}
        assert plan.rows["limit"] == [1, 3]
        for b, r in batch.items():
            assert plan.source[b] == (r.stages[-1] if r.stages else None)
            assert ("limit" in r.stages) == (r.ceiling > 0)
            if r.ceiling > 0:  # the last float stage: only the conversion and the framing stand behind it
                at = r.stages.index("limit")
                assert set(r.stages[:at]) <= FLOATS and set(r.stages[at + 1:]) <= {"resample", "flac"}
        # slot 0 skips the stage but a later stage reads its rows: passed through; the plain slot never is
        assert plan.through["limit"] == ([0] if set(batch[0].stages) & {"resample", "flac"} else [])
        assert ("limit" in plan.host) == any(r.stages and r.stages[-1] == "limit" for r in batch.values())
        for s in FLOATS & set(plan.through):  # the float stages in front pass a limited slot through where it skips them
            assert all(b in plan.through[s] or s in batch[b].stages for b in (1, 3))


def test_plans_without_a_limited_slot_are_todays():
    def todays(routes):  # plan_pass as it was before the stage existed, over TRIM_ORDER
        order = route.TRIM_ORDER
        paths = {b: tuple(s for s, o in zip(order, (r.trims, r.segmented, r.loudness is not None, r.speed_q != 65536, r.watermark_gain > 0.0,
                                                    r.enc != 0, r.flac)) if o) for b, r in routes.items()}
        rows = {s: [b for b, p in paths.items() if s in p] for s in order}
        stages = [s for s in order if rows[s]]
        through = {s: [b for b, p in paths.items() if p and s not in p and order.index(p[-1]) > order.index(s)]
                   for s in route.TRIM_FLOAT_STAGES if rows[s]}
        source = {b: (p[-1] if p else None) for b, p in paths.items()}
        return stages, {s: rows[s] for s in stages}, through, source, [s for s in stages if s in source.values()]

    for c1, c2, loud, mark, trim in itertools.product(COMBOS, COMBOS, (None, -20.0), (0.0, 0.05), (False, True)):
        routes = {0: _route(*c1, trim=trim), 1: route.SlotRoute(), 2: _route(*c2, loudness=loud, watermark_gain=mark)}
        plan = route.plan_pass(routes)
        assert (plan.stages, plan.rows, plan.through, plan.source, plan.host) == todays(routes)
        assert "limit" not in plan.stages and "limit" not in plan.rows and "limit" not in plan.through and "limit" not in plan.host


def test_converter_makes_no_limiter_until_a_slot_asks(monkeypatch):
    import torch

    made = []

    class Stage:
        def __init__(self, device, batch):
            made.append("limiter")

        def reset_slots(self, slots, ceilings):
            made.append(("reset", list(slots), list(ceilings)))

        def close(self):
            made.append("close")

    monkeypatch.setattr(route, "PeakLimiter", Stage)
    conv = route.StreamConverter(torch.device("cpu"), 4, 1920)
    conv.reset_slots([0, 1], [None, None], [None, None])
    conv.reset_slots([0, 1], [None, None], [None, None], limit=[None, 0.0])
    assert made == [] and conv.lim is None and not conv.converts(0) and conv.ends([0, 1]) == (False, False)
    c = LM.ceiling_of_db(-3.0)
    conv.reset_slots([1], [None], [None], limit=[c])
    assert made == ["limiter", ("reset", [1], [c])] and conv.converts(1) and not conv.converts(0)
    assert conv.routes[1].ceiling == c and conv.ends([0, 1]) == (True, False) and conv.ends([0]) == (False, False)
    assert conv.plan([0, 1]).stages == ["limit"] and conv.plan([0]).stages == [] and conv.plan([0, 1]).host == ["limit"]
    conv.reset_slots([1], [None], [None])  # the slot's next tenant does not ask: the stage switches it off
    assert made[-1] == ("reset", [1], [0.0]) and not conv.converts(1)
    conv.close()
    assert made[-1] == "close" and conv.lim is None


# ------------------------------------------------------------------------------- settings and HTTP
def test_setting_default_and_range():
    from pydantic import ValidationError

    from smoltts_amd.server.settings import ServerSettings

    assert ServerSettings(checkpoint_dir="x").peak_limit_db is None
    assert ServerSettings(checkpoint_dir="x", peak_limit_db=-1).peak_limit_db == -1.0
    assert ServerSettings(**ServerSettings(checkpoint_dir="x", peak_limit_db=-12.0).model_dump()).peak_limit_db == -12.0
    for bad in (0.1, -12.5, "loud"):
        with pytest.raises(ValidationError):
            ServerSettings(checkpoint_dir="x", peak_limit_db=bad)


class _LimitTTS:
    """A model that limits with the numpy model when asked to, and records the keywords it is called with."""
    sampling_rate = 24000

    def __init__(self):
        self.calls = []
        self.last_peak_reduction_db = None

    def __call__(self, text, voice="heart", **kw):
        parse_request(text, **kw)
        self.calls.append(("call", voice, dict(kw)))
        x = driven(1, 12.0)
        self.last_peak_reduction_db = None
        if kw.get("peak_limit_db") is not None:
            x, g = LM.limit(x, kw["peak_limit_db"])
            self.last_peak_reduction_db = LM.reduction_db(g)
        return x

    def stream(self, text, voice="heart", **kw):
        if not isinstance(text, str):
            text = "".join(t for t in text if isinstance(t, str))
        parse_request(text, stream=True, **{k: v for k, v in kw.items() if k != "segment"})
        self.calls.append(("stream", voice, dict(kw)))
        x = driven(1, 12.0)
        if kw.get("peak_limit_db") is None:
            yield from (x[i:i + 1920] for i in range(0, x.size, 1920))
            return
        st = LM.StreamState(kw["peak_limit_db"])
        for i in range(0, x.size, 1920):
            yield st.process(x[i:i + 1920], last=i + 1920 >= x.size)


def _client(model, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    app = create_app(model, settings=settings)
    return TestClient(app), app.state.tts_core


def test_route_bodies_carry_the_field_and_answer_the_header():
    from smoltts_amd.server.wav import pcm_to_wav_bytes

    model = _LimitTTS()
    c, _ = _client(model)
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert r.status_code == 200 and "x-peak-reduction-db" not in r.headers and model.calls[-1] == ("call", "sky", {})
    want, g = LM.limit(driven(1, 12.0), -3.0)
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "peak_limit_db": -3.0})
    assert r.status_code == 200 and model.calls[-1] == ("call", "sky", {"peak_limit_db": -3.0})
    assert r.headers["x-peak-reduction-db"] == f"{LM.reduction_db(g):.2f}" and float(r.headers["x-peak-reduction-db"]) > 0
    assert r.content == pcm_to_wav_bytes(want, 24000)
    r = c.post("/v1/text-to-speech/sky", json={"text": "hi", "peak_limit_db": -3, "loudness": -20.0})
    assert r.status_code == 200 and model.calls[-1] == ("call", "sky", {"peak_limit_db": -3.0, "loudness": -20.0})
    assert r.headers["x-peak-reduction-db"] == f"{LM.reduction_db(g):.2f}"
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "hi", "peak_limit_db": -3.0})
    assert r.status_code == 200 and "x-peak-reduction-db" not in r.headers and model.calls[-1] == ("stream", "sky", {"peak_limit_db": -3.0})
    assert np.array_equal(bits(np.frombuffer(r.content, np.float32)), bits(want))
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "response_format": "pcm", "peak_limit_db": -3.0})
    assert r.status_code == 200 and model.calls[-1] == ("stream", "sky", {"peak_limit_db": -3.0})
    assert np.array_equal(np.frombuffer(r.content, "<i2"), np.rint(np.clip(want, -1, 1) * np.float32(32767.0)).astype("<i2"))
    # under the ceiling: the header says 0.00
    class Quiet(_LimitTTS):
        def __call__(self, text, voice="heart", **kw):
            x, g = LM.limit(driven(1, 0.0), kw["peak_limit_db"])
            self.last_peak_reduction_db = LM.reduction_db(g)
            return x

    cq, _ = _client(Quiet())
    r = cq.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "peak_limit_db": 0})
    assert r.status_code == 200 and r.headers["x-peak-reduction-db"] == "0.00"
    for route_, body in (("/v1/audio/speech", {"input": "hi", "voice": "sky"}), ("/v1/text-to-speech/sky", {"text": "hi"}),
                         ("/v1/text-to-speech/sky/stream", {"text": "hi"}),
                         ("/v1/audio/speech", {"input": "hi", "voice": "sky", "response_format": "flac"})):
        for bad in (0.5, -13):
            r = c.post(route_, json=dict(body, peak_limit_db=bad))
            assert r.status_code == 400 and "peak_limit_db" in r.json()["detail"], (route_, bad, r.text)


def test_stream_input_route_carries_the_field():
    import json

    model = _LimitTTS()
    c, _ = _client(model)
    body = json.dumps({"peak_limit_db": -3.0}) + "\n" + json.dumps({"text": "Hello there. "}) + "\n" + json.dumps({"text": ""}) + "\n"
    r = c.post("/v1/text-to-speech/sky/stream-input", content=body)
    assert r.status_code == 200, r.text
    assert model.calls[-1][0] == "stream" and model.calls[-1][2].get("peak_limit_db") == -3.0
    r = c.post("/v1/text-to-speech/sky/stream-input", content=json.dumps({"peak_limit_db": 3.0}) + "\n")
    assert r.status_code == 400 and "peak_limit_db" in r.text


def test_server_setting_is_the_default_when_the_body_omits_the_field():
    model = _LimitTTS()
    c, _ = _client(model, {"peak_limit_db": -6.0})
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky"})
    assert r.status_code == 200 and model.calls[-1] == ("call", "sky", {"peak_limit_db": -6.0}) and float(r.headers["x-peak-reduction-db"]) > 0
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "peak_limit_db": -1.0})
    assert model.calls[-1] == ("call", "sky", {"peak_limit_db": -1.0})
    r = c.post("/v1/audio/speech", json={"input": "hi", "voice": "sky", "peak_limit_db": None})  # null: off
    assert r.status_code == 200 and model.calls[-1] == ("call", "sky", {}) and "x-peak-reduction-db" not in r.headers
    r = c.post("/v1/text-to-speech/sky/stream", json={"text": "hi"})
    assert model.calls[-1] == ("stream", "sky", {"peak_limit_db": -6.0})


# ------------------------------------------------------------------------------- the C interface
def test_header_exports_are_bound_and_the_abi_is_nine():
    header = (ROOT / "include" / "smoltts_hip.h").read_text()
    names = sorted(set(re.findall(r"\b(smoltts_limiter_\w+)\s*\(", header)))
    assert names == sorted(f"smoltts_limiter_{s}" for s in ("bytes", "table_doubles", "create", "destroy", "out_samples", "reset_slots",
                                                           "chunk", "apply", "slot_state"))
    assert all(n in abi.SIGNATURES for n in names)
    assert abi.SIGNATURES["smoltts_limiter_chunk"] == (abi.INT, "p p q i i p p p q p p")
    assert abi.SIGNATURES["smoltts_limiter_apply"] == (abi.INT, "p p i d p p p")
    assert abi.ABI_VERSION == 9 and re.search(r"#define\s+SMOLTTS_ABI_VERSION\s+9\b", header)
    from smoltts_amd.build import SOURCES

    assert "limiter.hip" in SOURCES and (ROOT / "smoltts_amd" / "csrc" / "limiter.hip").exists()


def test_library_exports_the_sizes():
    lib = abi.load_library()
    assert lib.smoltts_limiter_table_doubles() == 36 == LM.packed().size
    assert lib.smoltts_limiter_out_samples(0) == 126 and lib.smoltts_limiter_out_samples(61440) == 61440 + 126
    assert lib.smoltts_limiter_out_samples(61441) == 0 and lib.smoltts_limiter_out_samples(-1) == 0
    per_slot = 8 * 1440 + 24 + 4 * 126 + 8
    assert lib.smoltts_limiter_bytes(0) == 0 and lib.smoltts_limiter_bytes(4) >= 2 * 4 * per_slot + 36 * 8
    assert lib.smoltts_limiter_bytes(4) % 256 == 0
