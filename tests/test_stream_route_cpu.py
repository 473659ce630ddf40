"""The routing of the stream stages behind the codec, host side (no GPU, no library): ``engine.plan_pass`` over batches that mix
plain slots with every allowed combination of segments, speed, format and FLAC, checked against the rules the converter has
always followed; and ``StreamConverter.run`` executing a plan on stand-in stages (CPU tensors), with the per-slot snapshot a
pass keeps while its slots are restarted; and the stage table (``route.STAGE_TABLE``) as the single source of the routes, the
end markers and the calls of a pass over all eight stages."""
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

            run = chunk  # (the limiter's entry for rows of any width)

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
    for cls, width, count in (("SilenceTrimmer", 8, 11), ("LoudnessNormalizer", 0, 13), ("Watermarker", 0, 17), ("PeakLimiter", 126, 19)):
        monkeypatch.setattr(route, cls, stage(cls, width, count))
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
    assert [e[:2] for e in log] == [("create", "stretch"), ("reset", "stretch"), ("create", "resample"), ("reset", "resample"),
                                    ("create", "flac"), ("reset", "flac"), ("create", "seam"), ("reset", "seam")]  # (launch order)
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


# ------------------------------------------------------------------------------- the stage table
DECLARED = {"trim": {"seg_end", "last"}, "seam": {"seg_end", "last"}, "stretch": {"last"}, "limit": {"last"}, "loudness": set(),
            "watermark": set()}  # the end markers each float stage's class declares


def _every_route():
    """``COMBOS`` crossed with the trim (off, the ends, a pause cap), loudness, watermark and limiter on and off."""
    return [_route_of(c, trim=t, pause_blocks=p, loudness=ld, watermark_gain=g, ceiling=ce)
            for c, (t, p), ld, g, ce in itertools.product(COMBOS, ((False, 0), (True, 0), (False, 3)), (None, -20.0), (0.0, 0.05), (0.0, 0.5))]


def _route_of(combo, **kw):
    seg, q, fmt, fl = combo
    rate, enc = parse_stream_format(fmt)
    return route.SlotRoute(rate, enc, q, fl, segmented=seg, **kw)


def test_the_table_is_the_single_source():
    assert tuple(s.name for s in route.STAGE_TABLE) == route.LIMIT_ORDER
    assert tuple(s.name for s in route.STAGE_TABLE if s.fp32) == route.LIMIT_FLOAT_STAGES
    assert [s.attr for s in route.STAGE_TABLE] == ["tr", "sj", "ln", "ts", "wm", "lim", "rs", "fl"]
    assert {s.name: set(getattr(route, s.cls).END_MARKERS) for s in route.STAGE_TABLE if s.fp32} == DECLARED
    routes = _every_route()
    assert len(routes) == len(COMBOS) * 3 * 2 * 2 * 2
    for r in routes:  # the eight conditions as the route stated them before the table
        path = []
        if r.trim or r.pause_blocks > 0:
            path.append("trim")
        if r.segmented:
            path.append("seam")
        if r.loudness is not None:
            path.append("loudness")
        if r.speed_q != 65536:
            path.append("stretch")
        if r.watermark_gain > 0.0:
            path.append("watermark")
        if r.ceiling > 0.0:
            path.append("limit")
        if r.enc != ENC_OFF:
            path.append("resample")
        if r.flac:
            path.append("flac")
        assert r.stages == tuple(path)


def test_ends_of_every_one_and_two_slot_plan_follow_the_literal_rule():
    conv = engine.StreamConverter(torch.device("cpu"), 2, 1920)
    routes = _every_route()
    for r0, r1 in itertools.product(routes, routes):
        conv.routes[:] = [r0, r1]
        for slots in ([0], [0, 1]) if r1 is routes[0] else ([0, 1],):
            stages = conv.plan(slots).stages
            assert conv.ends(slots) == (any(s in stages for s in ("trim", "seam", "stretch", "limit", "flac")),
                                        "seam" in stages or "trim" in stages)


def test_a_pass_with_all_eight_stages_runs_in_table_order_with_each_stage_its_declared_markers(monkeypatch):
    """Slot 0 takes every stage, slot 1 is plain, slot 2 takes the loudness stage and the resampler: every other float stage
    passes it through."""
    from smoltts_amd import watermark as W

    log = []
    _stand_ins(monkeypatch, log)
    name_of = {"SilenceTrimmer": "trim", "LoudnessNormalizer": "loudness", "Watermarker": "watermark", "PeakLimiter": "limit"}
    conv = engine.StreamConverter(torch.device("cpu"), 3, 1920, watermark=W.Watermark(0x0123456789ABCDEF, -26.0))
    conv.reset_slots([0, 1, 2], ["pcm_16000", None, "ulaw_8000"], [32768, None, None], ["flac", None, None], [-20.0, None, -16.0],
                     None, [True, False, False], [(True, 0, None), None, None], [0.5, None, None])
    conv.start_segments([0], [480], [engine.SEAM_FIRST], [240])
    assert conv.routes[0].stages == route.LIMIT_ORDER and conv.routes[1].stages == () and conv.routes[2].stages == ("loudness", "resample")
    assert all(getattr(conv, s.attr) is not None for s in route.STAGE_TABLE) and conv.ends([0, 1, 2]) == (True, True)

    log.clear()
    pcm = torch.arange(3 * 1920, dtype=torch.float32).reshape(3, 1920)
    valid = torch.tensor([1920, 1900, 1800], dtype=torch.int32)
    last, seg_end = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    p = conv.run(pcm, 1920, valid, last=last, seg_end=seg_end)
    assert all(e[0] == "chunk" for e in log) and [name_of.get(e[1], e[1]) for e in log] == list(route.LIMIT_ORDER)
    assert p.plan.source == {0: "flac", 1: None, 2: "resample"} and list(p.dev) == ["resample", "flac"]
    src, width, seen = pcm, 1920, valid
    want_valid = {"trim": [11, 1900, 1800], "seam": [7, 1900, 1800], "loudness": [13, 13, 13], "stretch": [5, 13, 13],
                  "watermark": [17, 13, 13], "limit": [19, 13, 13]}  # (a stage that passes no slot through hands on its counts)
    for (_, cls, a, k), grows in zip(log[:6], (8, 16, 0, 32, 0, 126)):
        s = name_of.get(cls, cls)
        assert len(a) == 4 and a[0] is src and a[1] == width and a[2].shape == (3, width + grows) and a[3].shape == (3,)
        assert set(k) == {"valid"} | DECLARED[s] and k["valid"].tolist() == seen.tolist()
        assert k.get("last", last) is last and k.get("seg_end", seg_end) is seg_end
        if s != "loudness":
            assert torch.equal(a[2][2, :width], src[2])  # passed through
        src, width, seen = a[2], width + grows, torch.tensor(want_valid[s], dtype=torch.int32)
    assert width == 1920 + 8 + 16 + 32 + 126
    rs_call, flac_call = log[6:]
    rs_out, rs_counts = p.dev["resample"]
    assert rs_call[2][0] is src and rs_call[2][1] == width and rs_call[2][2] is rs_out and rs_call[2][3] is rs_counts and len(rs_call[2]) == 4
    assert set(rs_call[3]) == {"valid"} and rs_call[3]["valid"].tolist() == [19, 13, 13]
    fout, fsizes = p.dev["flac"]
    assert flac_call[2][0] == 3 and flac_call[2][1] is fout and flac_call[2][2] is fsizes and len(flac_call[2]) == 3
    k = flac_call[3]
    assert set(k) == {"pcm", "n_in", "valid", "s16", "s16_counts", "last"}
    assert k["pcm"] is src and k["n_in"] == width and k["valid"].tolist() == [19, 13, 13] and k["last"] is last
    assert k["s16"] is rs_out and k["s16_counts"] is rs_counts  # (the framed slot converts: FLAC reads the resampler's int16)
    conv.close()
    assert all(getattr(conv, s.attr) is None for s in route.STAGE_TABLE)


def test_the_shared_chunk_refuses_an_end_marker_its_stage_does_not_declare():
    from types import SimpleNamespace

    from smoltts_amd import stages

    class Bare(stages._FloatStage):  # no device: the C call is recorded
        C_NAME = "bare"

        def __init__(self):
            self.B, self.calls = 2, []
            self.lib = SimpleNamespace(smoltts_bare_out_samples=lambda n_in: n_in + 4)

        def _call(self, suffix, *args):
            self.calls.append((suffix, args))

    class Ending(Bare):
        END_MARKERS = ("last",)

    pcm, out, counts = torch.zeros(2, 16), torch.zeros(2, 20), torch.zeros(2, dtype=torch.int32)
    flag = torch.ones(2, dtype=torch.int32)
    st = Bare()
    assert st.END_MARKERS == ()
    with pytest.raises(AssertionError, match="Bare"):
        st.chunk(pcm, 16, out, counts, last=flag)
    with pytest.raises(AssertionError):
        st.chunk(pcm, 16, out, counts, seg_end=flag)
    assert st.calls == []
    st.chunk(pcm, 16, out, counts, valid=flag, last=None)
    assert st.calls == [("chunk", (pcm.data_ptr(), 16, 2, 16, flag.data_ptr(), out.data_ptr(), 20, counts.data_ptr()))]
    st = Ending()
    st.chunk(pcm, 16, out, counts, last=flag)
    st.chunk(pcm, 16, out, counts)
    assert [c[1][5] for c in st.calls] == [flag.data_ptr(), None] and all(len(c[1]) == 9 for c in st.calls)
    with pytest.raises(AssertionError):
        st.chunk(pcm, 16, out, counts, seg_end=flag, last=flag)
