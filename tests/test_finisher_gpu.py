"""``stages.Finisher`` on the GPU against the whole-utterance helpers composed by hand with fresh per-call stages, bit for bit,
on synthetic PCM (no model): every option on, the cap rule, three segments with an empty one, a row past ``trim.MAX_CALL``,
no option at all, one finisher reused across utterances and keys, and the head / stretch / tail split.

The base signal is 3 600 zeros, a 0.35 s two-tone burst at amplitude 0.5, 7 200 zeros, a second burst, 3 600 zeros: 31 200
samples at 24 kHz.  It has complete 400 ms blocks for the loudness gate, leading and trailing silence for the trim, and one
pause longer than 0.1 s."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from smoltts_amd import loudness, stages, trim  # noqa: E402
from smoltts_amd import watermark as W  # noqa: E402
from smoltts_amd.request import parse_request  # noqa: E402
from smoltts_amd.seam import segment_flags  # noqa: E402

KEY = W.Watermark(0x0123456789ABCDEF, -26.0)
ALL = dict(trim_silence=True, max_pause_s=0.1, loudness=-10.0, speed=1.25, peak_limit_db=-6.0)
CAP_TARGET = -6.0  # (the base signal measures -15.0 LUFS with a peak of 0.52: this target's gain of 2.8 takes the peak past -1 dBFS)


def _base() -> np.ndarray:
    rng = np.random.default_rng(20)
    t = np.arange(8400) / 24000.0

    def burst():
        return (0.25 * (np.sin(2 * np.pi * 220 * t) + np.sin(2 * np.pi * 550 * t)) + 0.01 * rng.standard_normal(t.size)).astype(np.float32)

    def zeros(n):
        return np.zeros(n, np.float32)

    return np.concatenate([zeros(3600), burst(), zeros(7200), burst(), zeros(3600)])


BASE = _base()


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _opts(**kw):
    return parse_request("x", False, **kw)


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _compose_plain(device, opts, key):
    """Every option of ``ALL`` by hand, each helper with a stage of its own: (samples, trimmed s, gain dB, reduction dB)."""
    y = stages.trim_pcm(BASE, 3, device, *opts.trim_route)
    trimmed_s = 0.0 + (BASE.size - y.size) / 24000.0
    y, g = stages.loudness_normalize(y, opts.loudness, device, with_gain=True, cap=False)
    y = stages.stretch_pcm(y, opts.speed_q, device)
    y = stages.watermark_embed(y, key, device)
    y, reduction = stages.peak_limit(y, opts.peak_limit_db, device)
    return y, trimmed_s, loudness.gain_db(g), reduction


@pytest.fixture(scope="module")
def plain(device):
    """Case 1's reference, computed once."""
    want = _compose_plain(device, _opts(**ALL), KEY)
    want[0].setflags(write=False)
    return want


def _segmented(device):
    """Case 3: (segments, options, plan, the composition by hand)."""
    opts = _opts(trim_silence=True, max_pause_s=0.1, loudness=-16.0)
    plan = parse_request("One. Two. Three.", False, segment={"max_bytes": 6}).plan
    assert len(plan.segs) == 3
    segments = [BASE, np.zeros(0, np.float32), BASE[::-1].copy()]
    cut = [stages.trim_pcm(x, segment_flags(k, 3), device, *opts.trim_route) for k, x in enumerate(segments)]
    trimmed_s = 0.0
    for x, y in zip(segments, cut):
        trimmed_s += (x.size - y.size) / 24000.0
    y = stages.seam_join(cut, plan.pauses, device, lead=plan.lead, trail=plan.trail)
    y, g = stages.loudness_normalize(y, opts.loudness, device, with_gain=True)
    return segments, opts, plan, (y, trimmed_s, loudness.gain_db(g), None)


def _check(got, want):
    assert _same(got[0], want[0])
    assert tuple(got[1:]) == tuple(want[1:])


def test_every_option_on_is_the_helpers_composed_by_hand(device, plain):
    fin = stages.Finisher(device)
    try:
        got = fin([BASE], _opts(**ALL), KEY)
    finally:
        fin.close()
    print(f"{BASE.size} -> {got[0].size} samples; trimmed s, gain dB, reduction dB: {got[1:]} (by hand {plain[1:]})")
    assert plain[3] > 0 and plain[1] > 0  # (the limiter and the trim both had work)
    _check(got, plain)


def test_the_loudness_gain_is_capped_exactly_without_a_limiter(device):
    p, peak = loudness.measure_power(BASE)
    assert loudness.static_gain(CAP_TARGET, p, peak, True) < loudness.static_gain(CAP_TARGET, p, peak, False)
    capped, g_cap = stages.loudness_normalize(BASE, CAP_TARGET, device, with_gain=True, cap=True)
    free, g_free = stages.loudness_normalize(BASE, CAP_TARGET, device, with_gain=True, cap=False)
    assert g_cap < g_free and not _same(capped, free)
    fin = stages.Finisher(device)
    try:
        _check(fin([BASE], _opts(loudness=CAP_TARGET), None), (capped, 0.0, loudness.gain_db(g_cap), None))
        y, reduction = stages.peak_limit(free, -6.0, device)
        _check(fin([BASE], _opts(loudness=CAP_TARGET, peak_limit_db=-6.0), None), (y, 0.0, loudness.gain_db(g_free), reduction))
    finally:
        fin.close()


def test_three_segments_the_middle_one_empty(device):
    segments, opts, plan, want = _segmented(device)
    fin = stages.Finisher(device)
    try:
        got = fin(segments, opts, None, plan)
    finally:
        fin.close()
    assert want[1] > 0 and want[0].size > 0
    _check(got, want)


def test_a_row_past_the_trims_call_size_on_a_held_stage(device):
    n = trim.MAX_CALL + 2400
    row = np.tile(BASE, -(-n // BASE.size))[:n].copy()
    opts = _opts(trim_silence=True, max_pause_s=0.1, peak_limit_db=-6.0)
    y = stages.trim_pcm(row, 3, device, *opts.trim_route)
    want = stages.peak_limit(y, -6.0, device)
    fin = stages.Finisher(device)
    try:
        first = fin([row], opts, None)
        again = fin([row], opts, None)  # (the held trimmer's second utterance)
    finally:
        fin.close()
    assert 0 < y.size < n
    for got in (first, again):
        _check(got, (want[0], 0.0 + (n - y.size) / 24000.0, None, want[1]))


def test_no_option_makes_no_stage(device, monkeypatch):
    made = []
    real = stages._Stage.__init__
    monkeypatch.setattr(stages._Stage, "__init__", lambda self, *a, **k: (made.append(type(self)), real(self, *a, **k))[1])
    fin = stages.Finisher(device)
    opts = _opts()
    assert not fin.needed(opts, None) and fin.needed(opts, KEY) and fin.needed(_opts(speed=1.25), None)
    got = fin([BASE], opts, None)
    assert _same(got[0], BASE) and tuple(got[1:]) == (0.0, None, None)
    assert not fin.held and not made
    fin.close()


def test_one_finisher_reused_across_utterances_and_keys(device, plain):
    segments, seg_opts, plan, seg_want = _segmented(device)
    opts = _opts(**ALL)
    other = W.Watermark(0x0FEDCBA987654321, -26.0)
    fin = stages.Finisher(device)
    try:
        first = fin([BASE], opts, KEY)
        between = fin(segments, seg_opts, None, plan)
        third = fin([BASE], opts, KEY)
        marker = fin.held[stages.Watermarker]
        fourth = fin([BASE], opts, other)
        assert fin.held[stages.Watermarker] is not marker and fin.held[stages.Watermarker].wm is other
    finally:
        fin.close()
    _check(first, plain)
    _check(between, seg_want)
    _check(third, first)
    want = _compose_plain(device, opts, other)
    assert not _same(want[0], plain[0])  # (the other key's mark is another signal)
    _check(fourth, want)


def test_head_stretch_tail_is_the_call(device, plain):
    opts = _opts(**ALL)
    fin = stages.Finisher(device)
    try:
        y, trimmed_s, gain = fin.head([BASE], opts)
        y = stages.stretch_pcm(y, opts.speed_q, device)
        y, reduction = fin.tail(y, opts, KEY)
        whole = fin([BASE], opts, KEY)
    finally:
        fin.close()
    _check((y, trimmed_s, gain, reduction), whole)
    _check(whole, plain)
