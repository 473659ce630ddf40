"""The routing of the stream stages behind the codec, host side (no GPU, no library): ``engine.plan_pass`` over batches that mix
plain slots with every allowed combination of segments, speed, format and FLAC, checked against the rules the converter has
always followed; and ``StreamConverter.run`` executing a plan on stand-in stages (CPU tensors), with the per-slot snapshot a
pass keeps while its slots are restarted."""
import itertools

import numpy as np
import pytest
import torch

from smoltts_amd import engine, route
from smoltts_amd.formats import ENC_OFF, parse_stream_format

FORMATS = ("pcm_24000", "pcm_16000", "ulaw_8000")
# (segmented, speed_q, format, flac): FLAC frames PCM only
COMBOS = [(seg, q, f, fl) for seg, q, f, fl in itertools.product((False, True), (65536, 32768), FORMATS, (False, True))
          if not (fl and f.startswith("ulaw"))]
PLAIN = (False, 65536, "pcm_24000", False)


def _route(seg, q, fmt, fl):
    rate, enc = parse_stream_format(fmt)
    return engine.SlotRoute(rate, enc, q, fl, segmented=seg)


def _expect(batch):
    """What a pass over ``batch`` ({slot: combo}) launches, reads and copies, by the converter's rules stated slot set by slot
    set: the seam stage first, the stretch, the resampler, then FLAC."""
    smd = [b for b, c in batch.items() if c[0]]
    spd = [b for b, c in batch.items() if c[1] != 65536]
    fmt = [b for b, c in batch.items() if parse_stream_format(c[2])[1] != ENC_OFF]
    flc = [b for b, c in batch.items() if c[3]]
    stages = [s for s, rows in zip(engine.STAGES, (smd, spd, fmt, flc)) if rows]
    source = {}
    for b in batch:
        path = [s for s, rows in zip(engine.STAGES, (smd, spd, fmt, flc)) if b in rows]
        source[b] = path[-1] if path else None
    through = {}
    if smd:  # a slot that skips the seam but needs a later stage has its codec rows passed through
        through["seam"] = sorted({b for b in fmt + spd + flc if b not in smd})
    if spd:
        through["stretch"] = sorted({b for b in fmt + flc if b not in spd})
    host = set()
    if any(b not in fmt and b not in flc for b in spd):
        host.add("stretch")  # a stretched slot that goes to no later stage
    if any(b not in flc for b in fmt):
        host.add("resample")  # a converted slot that is not framed
    if any(b not in fmt and b not in flc and b not in spd for b in smd):
        host.add("seam")  # a joined slot that goes to no later stage
    if flc:
        host.add("flac")
    return stages, source, through, host


def _check_plan(batch):
    plan = engine.plan_pass({b: _route(*c) for b, c in batch.items()})
    stages, source, through, host = _expect(batch)
    assert plan.stages == stages
    assert plan.source == source
    assert {s: sorted(rows) for s, rows in plan.through.items()} == through
    assert set(plan.host) == host and plan.host == [s for s in plan.stages if s in host]
    assert all(plan.rows[s] == [b for b in batch if s in _route(*batch[b]).stages] for s in stages)


def test_combos_cover_every_allowed_route():
    assert len(COMBOS) == 20 and PLAIN in COMBOS


@pytest.mark.parametrize("c1", COMBOS, ids=str)
def test_plan_of_every_pair_beside_plain_slots(c1):
    for c2 in COMBOS:
        _check_plan({0: PLAIN, 1: c1, 2: PLAIN, 3: c2})


def test_plan_of_every_combination_in_one_batch():
    batch = {}
    for k, c in enumerate(COMBOS):
        batch[2 * k], batch[2 * k + 1] = c, PLAIN
    _check_plan(batch)
    _check_plan(dict(reversed(list(batch.items()))))


def test_plain_slots_plan_nothing():
    plan = engine.plan_pass({b: engine.SlotRoute() for b in range(4)})
    assert plan.stages == [] and plan.host == [] and set(plan.source.values()) == {None}
    assert engine.plan_pass({}).stages == []


# ------------------------------------------------------------------------------- run on stand-in stages
def _stand_ins(monkeypatch, log):
    """Stage classes that record their calls and answer with CPU tensors: float stages emit ``width`` samples per row more than
    they read, with a fixed count, the resampler two bytes a sample, FLAC no frame."""
    slot_frames = engine.FlacEncoder.slot_frames

    def stage(name, width=0, count=0):
        class Stage:
            def __init__(self, *a):
                log.append(("create", name, a))

            def reset_slots(self, slots, *a):
                log.append(("reset", name, list(slots), a))

            def start_segments(self, slots, *a):
                log.append(("reset", name, list(slots), a))

            def new_outputs(self, batch, n):
                if name == "resample":
                    return torch.zeros(batch, 2 * n, dtype=torch.uint8), torch.zeros(batch, 2, dtype=torch.int32)
                if name == "flac":
                    return torch.zeros(batch, 64, dtype=torch.uint8), torch.zeros(batch, 2, 2, dtype=torch.int32)
                return torch.full((batch, n + width), -1.0), torch.full((batch,), count, dtype=torch.int32)

            def chunk(self, *a, **k):
                log.append(("chunk", name, a, k))

            def slot_bytes(self, out, counts, b, tail=False, enc=None):
                return ("bytes", b, enc)

            def close(self):
                pass

        Stage.slot_frames = staticmethod(slot_frames)
        return Stage

    monkeypatch.setattr(route, "SeamJoiner", stage("seam", 16, 7))
    monkeypatch.setattr(route, "TimeStretcher", stage("stretch", 32, 5))
    monkeypatch.setattr(route, "Resampler", stage("resample"))
    monkeypatch.setattr(route, "FlacEncoder", stage("flac"))
    for cls in ("SilenceTrimmer", "LoudnessNormalizer", "Watermarker", "PeakLimiter"):
        monkeypatch.setattr(route, cls, stage(cls))
    monkeypatch.setattr(route, "upload", lambda arrays, device: [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays])


def test_run_executes_the_plan_and_the_pass_keeps_its_routes(monkeypatch):
    from smoltts_amd.flac import stream_header

    log = []
    _stand_ins(monkeypatch, log)
    conv = engine.StreamConverter(torch.device("cpu"), 5, 1920)
    conv.reset_slots([0, 1, 2, 3], [None] * 4, [None] * 4)
    assert log == [] and not any(conv.converts(b) for b in range(5))  # plain streams: no stage, no call
    assert conv.run(torch.zeros(5, 1920), 1920, torch.zeros(5, dtype=torch.int32)) is None and log == []

    conv.reset_slots([1, 2, 4], ["pcm_16000", None, "pcm_24000"], [None, 32768, None], [None, None, "flac"])
    conv.start_segments([3], [480], [engine.SEAM_FIRST], [240])
    assert [e[:2] for e in log] == [("create", "resample"), ("create", "stretch"), ("create", "flac"), ("reset", "resample"),
                                    ("reset", "stretch"), ("reset", "flac"), ("create", "seam"), ("reset", "seam")]
    assert [conv.converts(b) for b in range(5)] == [False, True, True, True, True]
    assert conv.ends([0, 1]) == (False, False) and conv.ends([0, 2]) == (True, False) and conv.ends([4]) == (True, False)
    assert conv.ends([1, 3]) == (True, True)

    log.clear()
    pcm = torch.arange(5 * 1920, dtype=torch.float32).reshape(5, 1920)
    valid = torch.tensor([1920, 1900, 1800, 1700, 1600], dtype=torch.int32)
    p = conv.run(pcm, 1920, valid, last=torch.zeros(5, dtype=torch.int32), seg_end=torch.zeros(5, dtype=torch.int32))
    assert [e[1] for e in log] == ["seam", "stretch", "resample", "flac"]
    assert p.plan.source == {0: None, 1: "resample", 2: "stretch", 3: "seam", 4: "flac"}
    assert list(p.dev) == ["seam", "stretch", "resample", "flac"] and not p.converts(0)
    joined, stretched = p.dev["seam"][0], p.dev["stretch"][0]
    assert torch.equal(joined[[1, 2, 4], :1920], pcm[[1, 2, 4]])            # passed through the seam
    assert torch.equal(stretched[[1, 4], :1920 + 16], joined[[1, 4]])        # ... and the stretch
    seam_call, stretch_call, rs_call, flac_call = log
    assert stretch_call[2][0] is joined and rs_call[2][0] is stretched and rs_call[2][1] == 1920 + 16 + 32
    assert rs_call[3]["valid"].tolist() == [1920, 1900, 5, 7, 1600]      # each slot's count from its last float stage
    assert flac_call[3]["s16"] is None and flac_call[3]["pcm"] is stretched  # (the FLAC slot reads float32)

    conv.reset_slots([1, 2, 4], [None] * 3, [None] * 3)  # restarted before the pass is read
    assert not any(conv.converts(b) for b in (1, 2, 4))
    p.host = p.dev
    assert p.chunk(1, True) == ("bytes", 1, parse_stream_format("pcm_16000")[1])
    assert np.array_equal(p.chunk(2, False), stretched[2, :5].numpy()) and np.array_equal(p.chunk(3, False), joined[3, :7].numpy())
    assert p.chunk(4, False).size == 0  # the restarted slot's new stream is not owed the old stream's header

    conv.reset_slots([4], [None], [None], ["flac"])
    p = conv.run(pcm, 1920, valid, last=torch.zeros(5, dtype=torch.int32), slots=[4])
    p.host = p.dev
    assert p.chunk(4, False).tobytes() == stream_header(24000) and p.chunk(4, False).size == 0  # the header once per stream


# ------------------------------------------------------------------------------- a route from a request's options
def test_start_from_options_is_reset_slots_from_the_nine_lists(monkeypatch):
    """Every (speed, format, FLAC) of ``COMBOS`` crossed with trim, loudness, watermark and limiter on and off: ``start`` from
    the parsed requests leaves the routes ``reset_slots`` leaves from the nine lists (generation and owed header included), and
    creates and resets the stages in the same order with the same arguments.  (``segmented`` is ``start_segments``' to set.)"""
    from smoltts_amd import watermark as W
    from smoltts_amd.request import parse_request

    key = W.Watermark(0x0123456789ABCDEF, -26.0)
    cases = []
    for (_, q, fmt, fl), trim, loud, wm, lim in itertools.product(sorted(set((False,) + c[1:] for c in COMBOS)), (0, 1, 2), (0, 1, 2),
                                                                  (False, True), (False, True)):
        kw = dict(output_format=fmt, speed=q / 65536, container="flac" if fl else None)
        kw.update([{}, dict(trim_silence=True), dict(max_pause_s=0.3, silence_threshold_db=-40.0)][trim])
        kw.update([{}, dict(loudness=-20.0), dict(loudness=-16.0, loudness_start_gain_db=1.5)][loud])
        if lim:
            kw["peak_limit_db"] = -6.0
        cases.append((parse_request("x", stream=True, **kw), wm))
    assert len(cases) == 10 * 3 * 3 * 2 * 2
    B = 7  # more than one batch of slots, restarted case after case: every slot's generation grows
    logs, convs = ([], []), []
    for log in logs:
        _stand_ins(monkeypatch, log)
        convs.append(engine.StreamConverter(torch.device("cpu"), B, 1920, watermark=key))
    by_options, by_lists = convs
    for i in range(0, len(cases), B - 2):
        batch = cases[i:i + B - 2]
        slots = [(i + 3 * k) % B for k in range(len(batch))]
        opts, marked = [p for p, _ in batch], [wm for _, wm in batch]
        _stand_ins(monkeypatch, logs[0])
        by_options.start(slots, opts, marked)
        _stand_ins(monkeypatch, logs[1])
        by_lists.reset_slots(slots, [p.output_format for p in opts], [p.speed_q for p in opts], [p.container for p in opts],
                             [p.loudness for p in opts], [p.start_gain_db for p in opts], marked,
                             [p.trim_route for p in opts], [p.ceiling for p in opts])
        assert by_options.routes == by_lists.routes
        assert all(r.gen >= 1 and r.head_owed == r.flac for r in (by_options.routes[b] for b in slots))
    assert logs[0] == logs[1] and len(logs[0]) > len(cases)
    assert {e[1] for e in logs[0] if e[0] == "create"} == {"SilenceTrimmer", "LoudnessNormalizer", "Watermarker", "PeakLimiter",
                                                            "resample", "stretch", "flac"}
    routes = {by_options.routes[b] for b in range(B)}
    assert max(r.gen for r in routes) > 1 and any(r.watermark_gain == key.gain for r in routes)
    # a converter without a key refuses a marked slot from either entry point, and starts nothing
    bare = engine.StreamConverter(torch.device("cpu"), 2, 1920)
    for start in (lambda: bare.start([0], [cases[0][0]], [True]), lambda: bare.reset_slots([0], [None], [None], watermark=[True])):
        with pytest.raises(ValueError, match="has no key"):
            start()
    assert bare.routes == [engine.SlotRoute()] * 2
    bare.start([1], [parse_request("x", stream=True)])
    assert bare.routes[1] == engine.SlotRoute(gen=1) and not bare.converts(1)
