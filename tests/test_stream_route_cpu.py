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
                log.append(("create", name))

            def reset_slots(self, slots, *a):
                log.append(("reset", name))

            def start_segments(self, slots, *a):
                log.append(("reset", name))

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
