"""``stages.Finisher``, host side (no GPU, no library): with the creation method and the six whole-utterance functions replaced
by recorders, every subset of the options, plain and segmented, runs exactly its stages in the one order, each segment with
its flags, the loudness gain capped exactly when no limiter follows, and an option that is off makes no stage."""
import itertools

import numpy as np
import pytest

from smoltts_amd import stages
from smoltts_amd.request import parse_request
from smoltts_amd.seam import segment_flags

OPTIONS = ("trims", "loudness", "speed", "mark", "limit")
KEYWORDS = {"trims": dict(trim_silence=True, max_pause_s=0.1), "loudness": dict(loudness=-10.0), "speed": dict(speed=1.25),
            "limit": dict(peak_limit_db=-6.0), "mark": {}}
CLASS_OF = {"trims": stages.SilenceTrimmer, "seam": stages.SeamJoiner, "loudness": stages.LoudnessNormalizer,
            "speed": stages.TimeStretcher, "mark": stages.Watermarker, "limit": stages.PeakLimiter}
KEY = object()  # (the recorders never look into the key)
SUBSETS = [frozenset(c) for n in range(len(OPTIONS) + 1) for c in itertools.combinations(OPTIONS, n)]


class _Stand:
    """What ``Finisher._make`` returns here: the class and arguments it was asked for."""

    def __init__(self, cls, *args):
        self.cls, self.args, self.wm, self.closed = cls, args, (args[0] if args else None), False

    def close(self):
        self.closed = True


@pytest.fixture
def recorded(monkeypatch):
    """(calls, made): every call of a whole-utterance function as (name, what the test looks at), every stage made.  Each
    function hands on an array one sample shorter than it was given, so that the order shows in the data too."""
    calls, made = [], []

    def make(self, cls, *args):
        made.append(cls)
        return _Stand(cls, *args)

    def trim_pcm(pcm, flags, device, trim=True, pause_blocks=0, thr=None, held=None):
        calls.append(("trims", flags, (trim, pause_blocks, thr), held.cls))
        return pcm[1:]

    def seam_join(segments, pauses, device, lead=0, trail=0, held=None):
        calls.append(("seam", [s.size for s in segments], (list(pauses), lead, trail), held.cls))
        return np.concatenate(segments)[1:]

    def loudness_normalize(pcm, target, device, with_gain=False, cap=True, held=None):
        calls.append(("loudness", target, (with_gain, cap), held.cls))
        return pcm[1:], 2.0

    def stretch_pcm(pcm, speed_q, device, held=None):
        calls.append(("speed", speed_q, pcm.size, held.cls))
        return pcm[1:]

    def watermark_embed(pcm, wm, device, held=None):
        calls.append(("mark", wm, held.wm, held.cls))
        return pcm[1:]

    def peak_limit(pcm, peak_limit_db, device, held=None):
        calls.append(("limit", peak_limit_db, pcm.size, held.cls))
        return pcm[1:], 1.5

    monkeypatch.setattr(stages.Finisher, "_make", make)
    for f in (trim_pcm, seam_join, loudness_normalize, stretch_pcm, watermark_embed, peak_limit):
        monkeypatch.setattr(stages, f.__name__, f)
    return calls, made


def _request(on, segmented):
    kw = {k: v for name in on for k, v in KEYWORDS[name].items()}
    req = parse_request("One. Two. Three.", False, **kw, **({"segment": {"max_bytes": 6}} if segmented else {}))
    assert (req.plan is not None) == segmented and (not segmented or len(req.plan.segs) == 3)
    return req


@pytest.mark.parametrize("segmented", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("on", SUBSETS, ids=lambda s: "+".join(sorted(s)) or "none")
def test_the_options_that_are_on_run_in_the_one_order(recorded, on, segmented):
    from smoltts_amd.loudness import gain_db

    calls, made = recorded
    req = _request(on, segmented)
    mark = KEY if "mark" in on else None
    n = 3 if segmented else 1
    segments = [np.arange(100 * (k + 1), dtype=np.float32) for k in range(n)]
    fin = stages.Finisher("dev")
    assert fin.needed(req, mark) == bool(on)
    pcm, trimmed_s, gain, reduction = fin(segments, req, mark, req.plan)

    order = [name for name in ("trims",) * n + ("seam", "loudness", "speed", "mark", "limit") if name in on or (name == "seam" and segmented)]
    assert [c[0] for c in calls] == order
    assert made == [CLASS_OF[name] for name in dict.fromkeys(order)] and set(fin.held) == set(made)
    assert all(c[3] is CLASS_OF[c[0]] for c in calls)  # every function got the stage of its own class
    by = {}
    for c in calls:
        by.setdefault(c[0], []).append(c)
    if "trims" in on:
        assert [c[1] for c in by["trims"]] == [segment_flags(k, n) for k in range(n)]
        assert all(c[2] == req.trim_route for c in by["trims"])
    assert trimmed_s == (sum([1 / 24000.0] * n) if "trims" in on else 0.0)
    if segmented:
        plan = req.plan
        assert by["seam"][0][1:3] == ([s.size - ("trims" in on) for s in segments], (list(plan.pauses), plan.lead, plan.trail))
    if "loudness" in on:
        assert by["loudness"][0][1:3] == (-10.0, (True, "limit" not in on))  # capped exactly when no limiter follows
    assert gain == (gain_db(2.0) if "loudness" in on else None)
    if "speed" in on:
        assert by["speed"][0][1] == req.speed_q
    if "mark" in on:
        assert by["mark"][0][1] is KEY and by["mark"][0][2] is KEY
    if "limit" in on:
        assert by["limit"][0][1] == -6.0
    assert reduction == (1.5 if "limit" in on else None)
    assert pcm.size == sum(s.size for s in segments) - len(order)  # (every call took its sample: none ran on another's input)
    if not on and not segmented:
        assert pcm is segments[0]


def test_head_and_tail_split_the_chain_at_the_stretch_and_a_new_key_remakes_the_watermarker(recorded):
    calls, made = recorded
    req = _request(frozenset(OPTIONS), True)
    segments = [np.arange(50, dtype=np.float32) for _ in range(3)]
    fin = stages.Finisher("dev")
    fin.head(segments, req, req.plan)
    assert [c[0] for c in calls] == ["trims"] * 3 + ["seam", "loudness"]
    del calls[:]
    fin.tail(segments[0], req, KEY)
    assert [c[0] for c in calls] == ["mark", "limit"] and stages.TimeStretcher not in fin.held
    first = fin.held[stages.Watermarker]
    fin.tail(segments[0], req, KEY)
    assert fin.held[stages.Watermarker] is first and made.count(stages.Watermarker) == 1  # the same key object: the same stage
    other = object()
    fin.tail(segments[0], req, other)
    assert first.closed and fin.held[stages.Watermarker].wm is other and made.count(stages.Watermarker) == 2
    held = list(fin.held.values())
    fin.close()
    assert all(s.closed for s in held) and not fin.held
