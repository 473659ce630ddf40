"""Silence trimming, host side (no GPU): the streaming model ``trim.TrimState`` against the offline rule ``trim.trim`` over
random chunkings and every boundary of the rule, request parsing, and the routing of the trim stage."""
import itertools

import numpy as np
import pytest

from smoltts_amd import engine, route, trim
from smoltts_amd.request import parse_request
from smoltts_amd.seam import BLOCK, FINAL, FIRST, THRESH
from test_watermark_cpu import COMBOS, _route

ALL_FLAGS = (0, FIRST, FINAL, FIRST | FINAL)


def _speech(n, rng, amp=0.3):
    x = rng.uniform(-amp, amp, n).astype(np.float32)
    x[::40] = amp
    return x


def _quiet(n, rng):
    return rng.uniform(-0.5, 0.5, n).astype(np.float32) * np.float32(2 ** -9)


def _runs(rng, lengths, head=0, tail=0, partial=0, partial_quiet=True):
    """Speech blocks separated by silent runs of ``lengths`` blocks, behind ``head`` and in front of ``tail`` silent blocks and a
    partial last block of ``partial`` samples."""
    parts = [_quiet(head * BLOCK, rng)]
    for r in lengths:
        parts += [_speech(BLOCK * int(rng.integers(1, 4)), rng), _quiet(r * BLOCK, rng)]
    parts += [_speech(BLOCK, rng), _quiet(tail * BLOCK, rng)]
    parts.append(_quiet(partial, rng) if partial_quiet else _speech(partial, rng))
    return np.concatenate(parts)


def _chunkings(n, rng, k=3):
    yield [n]
    for _ in range(k):
        sizes, left = [], n
        while left:
            m = int(min(left, rng.choice([0, 1, 7, 239, 240, 241, 1920, 7680, int(rng.integers(1, 20000))])))
            sizes.append(m)
            left -= m
        yield sizes + [0] * int(rng.integers(0 if sizes else 1, 2))


def _check(x, rng, flags, on, P, thr=THRESH, k=3):
    want = trim.trim(x, flags, on, P, thr)
    for sizes in _chunkings(x.size, rng, k):
        for last in (False, True):
            got, st = trim.trim_chunked(x, sizes, flags, on, P, thr, last=last)
            np.testing.assert_array_equal(got, want)
            s = st.state()
            assert s["n_in"] == s["judged"] == x.size and s["held"] == 0 and s["emitted"] == want.size and not st.open
            assert s["dropped_head"] + s["dropped_pause"] + s["dropped_tail"] == x.size - want.size
            assert min(s.values()) >= 0
    return want


def test_constants_and_parameters():
    assert (trim.HEAD_KEEP, trim.TAIL_KEEP, trim.HOLD, BLOCK) == (2, 10, 200, 240)
    assert trim.threshold(None) == THRESH == np.float32(2.0 ** -8) and trim.threshold(None).dtype == np.float32
    assert trim.threshold(-20.0) == np.float32(0.1) and trim.threshold(-72.0) == np.float32(10 ** -3.6)
    assert trim.pause_blocks(None) == 0 and trim.pause_blocks(0.1) == 10 and trim.pause_blocks(2.0) == 200
    assert trim.pause_blocks(0.11) == 11 and trim.pause_blocks(0.5) == 50
    assert [trim.tail_keep(P) for P in (0, 10, 11, 19, 20, 200)] == [10, 5, 6, 10, 10, 10]
    for bad in (-73.0, -5.0, float("nan")):
        with pytest.raises(ValueError, match="silence_threshold_db"):
            trim.threshold(bad)
    for bad in (0.09, 2.01, 0.0, float("nan")):
        with pytest.raises(ValueError, match="max_pause_s"):
            trim.pause_blocks(bad)
    for P in (-1, 5, 9, 201):
        with pytest.raises(ValueError):
            trim.trim(np.zeros(10, np.float32), P=P)


@pytest.mark.parametrize("seed", range(4))
def test_streaming_equals_offline_on_random_signals(seed):
    rng = np.random.default_rng(seed)
    for _ in range(6):
        parts = []
        for _ in range(int(rng.integers(1, 4))):
            parts.append(_quiet(int(rng.choice([0, 100, 240, 480, 720, 3000, 24000 - 7, 26000, 53000])), rng))
            parts.append(_speech(int(rng.integers(1, 5000)), rng))
        parts.append(_quiet(int(rng.choice([0, 239, 2400, 4800, 27000, 51000])), rng))
        x = np.concatenate(parts)
        flags, on = int(rng.choice(ALL_FLAGS)), bool(rng.integers(0, 2))
        P = int(rng.choice([0, 10, 11, 50, 200]))
        thr = THRESH if rng.random() < 0.5 else trim.threshold(float(rng.choice([-60.0, -40.0, -12.0])))
        _check(x, rng, flags, on, P, thr)


@pytest.mark.parametrize("P", [10, 11, 21, 200])
def test_pause_boundaries(P):
    rng = np.random.default_rng(P)
    a, c = (P + 1) // 2, P // 2
    for on, flags in itertools.product((False, True), ALL_FLAGS):
        for r in (1, 2, 3, P - 1, P, P + 1, 3 * P):
            x = _runs(rng, [r])
            y = _check(x, rng, flags, on, P, k=1)
            assert x.size - y.size == (max(r - P, 0) if r > P else 0) * BLOCK  # (head 0, tail 0: only case 3 can cut)
        r = P + 7
        x = _runs(rng, [r])
        y = trim.trim(x, flags, on, P)
        i = int(np.flatnonzero(np.abs(x) >= THRESH)[np.flatnonzero(np.diff(np.flatnonzero(np.abs(x) >= THRESH)) > BLOCK)[0]]) // BLOCK + 1
        np.testing.assert_array_equal(y, np.concatenate([x[:(i + a) * BLOCK], x[(i + r - c) * BLOCK:]]))  # first ceil, last floor


def test_head_boundaries():
    rng = np.random.default_rng(1)
    for r, P in itertools.product((0, 1, 2, 3, 9, 250), (0, 10, 11)):
        x = _runs(rng, [], head=r)
        for flags in ALL_FLAGS:
            y = _check(x, rng, flags, True, P, k=1)
            if flags & FIRST:
                np.testing.assert_array_equal(y, x[max(r - 2, 0) * BLOCK:])
            elif P and r > P:
                assert x.size - y.size == (r - P) * BLOCK
            else:
                np.testing.assert_array_equal(y, x)
            np.testing.assert_array_equal(_check(x, rng, flags, False, 0, k=1), x)


def test_tail_boundaries():
    rng = np.random.default_rng(2)
    for P in (0, 10, 11, 200):
        K = trim.tail_keep(P)
        for r in (0, 1, K - 1, K, K + 1, P - 1 if P else 3, P + 1, K + trim.HOLD - 1, K + trim.HOLD, K + trim.HOLD + 1, K + trim.HOLD + 40):
            for partial, pq in ((0, True), (100, True), (100, False)):
                x = _runs(rng, [], tail=r, partial=partial, partial_quiet=pq)
                for flags in ALL_FLAGS:
                    y = _check(x, rng, flags, True, P, k=1)
                    rr = r + (1 if partial and pq else 0)  # the silent partial block is the run's last block
                    if flags & FINAL and (pq or not partial):
                        keep = rr - trim.HOLD if (P == 0 and rr - K > trim.HOLD) else min(rr, K)
                        np.testing.assert_array_equal(y, x[:x.size - r * BLOCK - partial + keep * BLOCK][:x.size])
                        if P == 0:
                            assert x.size - y.size <= trim.HOLD * BLOCK  # never more than 2 s
                    elif P == 0:
                        np.testing.assert_array_equal(y, x)
                    else:  # no trimmed end: only the cap cuts, in the middle of the run
                        assert x.size - y.size == max(rr - P, 0) * BLOCK


def test_all_silent_empty_and_nan():
    rng = np.random.default_rng(3)
    for n in (0, 1, 239, 240, 241, 480, 700, 60000):
        x = _quiet(n, rng)
        for flags, P in itertools.product(ALL_FLAGS, (0, 10)):
            y = _check(x, rng, flags, True, P, k=1)
            if flags & FIRST:  # case 1 comes first: the last two blocks, the partial one counted
                nb = -(-n // BLOCK)
                np.testing.assert_array_equal(y, x[max(nb - 2, 0) * BLOCK:])
    x = _runs(rng, [30], head=5, tail=30)
    x[7 * BLOCK + 3] = np.nan  # a NaN inside the pause... wherever it falls, its block is not silence
    k = next(i for i in range(x.size // BLOCK) if trim.silent(x[i * BLOCK:(i + 1) * BLOCK], THRESH) and i > 8)
    x[k * BLOCK + 5] = np.nan
    for flags in ALL_FLAGS:
        y = _check(x, rng, flags, True, 10, k=2)
        assert np.isnan(y).sum() == 2
    q = _quiet(BLOCK * 4, rng)
    q[BLOCK + 1] = np.nan
    assert trim.trim(q).size == 4 * BLOCK - 0  # silent, NaN block, two silent: head keeps 1 of 1, the tail 2 of 2
    st = trim.TrimState()
    assert st.push(np.ones(10, np.float32)).size == 0  # a slot that is not open emits nothing
    st.start()
    assert st.push([]).size == 0 and st.push([], end=True).size == 0 and not st.open


def test_options_off_is_the_identity():
    rng = np.random.default_rng(4)
    x = _runs(rng, [1, 30, 250], head=40, tail=300, partial=17)
    for flags in ALL_FLAGS:
        np.testing.assert_array_equal(_check(x, rng, flags, False, 0), x)
        st = trim.TrimState()
        st.start(flags, False, 0)
        got = [st.push(x[i:i + 1000]) for i in range(0, x.size, 1000)]
        assert all(y.size % BLOCK == 0 for y in got) and st.held == 0  # nothing is ever held but the partial block
        assert sum(y.size for y in got) == x.size // BLOCK * BLOCK and st.part.size == x.size % BLOCK


def test_held_state_is_bounded_and_speech_leaves_at_once():
    rng = np.random.default_rng(5)
    x = _runs(rng, [400, 3], head=300, tail=500)
    for flags, on, P in itertools.product(ALL_FLAGS, (False, True), (0, 10, 11, 200)):
        st = trim.TrimState()
        st.start(flags, on, P)
        for i in range(0, x.size, 1111):
            piece = x[i:i + 1111]
            y = st.push(piece)
            assert st.held <= trim.HOLD * BLOCK and st.part.size < BLOCK
            done = x[:st.judged]
            loud = np.flatnonzero(np.abs(done) >= THRESH)
            if loud.size and loud[-1] >= st.judged - BLOCK:  # the newest complete block is speech: nothing stays held
                assert st.held == 0 and y.size >= BLOCK


def test_row_and_slab_sizes():
    """Host functions of the C library (no GPU): a row holds the call's samples behind a released hold; one call takes MAX_CALL."""
    lib = engine.load_library()
    hold = (trim.HOLD + 1) * BLOCK
    assert tuple(lib.smoltts_trim_out_samples(n) for n in (-1, 0, 1, 1920, 7680, trim.MAX_CALL, trim.MAX_CALL + 1)) == \
        (0, hold, hold + 1, hold + 1920, hold + 7680, hold + trim.MAX_CALL, 0)
    # two state halves per slot, each 96 bytes of counters and parameters and 48240 samples, the halves 256-byte aligned
    assert [lib.smoltts_trim_bytes(b) for b in (-1, 0, 1, 2, 32)] == [0, 0, 386560, 772608, 12355584]
    assert trim.MAX_CALL % BLOCK == 0 and trim.MAX_CALL >= 4 * 1920


# ------------------------------------------------------------------------------- request parsing
def test_request_parsing():
    o = parse_request("hi")
    assert (o.trim_silence, o.max_pause_s, o.silence_threshold_db) == (False, None, None) and not o.trims
    o = parse_request("hi", trim_silence=True)
    assert o.trim_silence and o.trims and o.pause_blocks == 0 and o.silence_thr == THRESH
    o = parse_request("hi", stream=True, max_pause_s=0.25, silence_threshold_db=-40)
    assert not o.trim_silence and o.trims and o.pause_blocks == 25 and o.silence_thr == np.float32(0.01)
    assert parse_request("hi", trim_silence=False, max_pause_s=None).trims is False
    for kw, msg in (({"trim_silence": 1}, "trim_silence must be true or false"),
                    ({"trim_silence": "yes"}, "trim_silence must be true or false"),
                    ({"max_pause_s": 0.05}, r"max_pause_s must be within \[0.1, 2\]"),
                    ({"max_pause_s": 2.5}, r"max_pause_s must be within \[0.1, 2\]"),
                    ({"max_pause_s": "x"}, "max_pause_s must be a number"),
                    ({"trim_silence": True, "silence_threshold_db": -80}, r"silence_threshold_db must be within \[-72, -6\]"),
                    ({"trim_silence": True, "silence_threshold_db": 0}, r"silence_threshold_db must be within \[-72, -6\]"),
                    ({"trim_silence": True, "silence_threshold_db": "x"}, "silence_threshold_db must be a number"),
                    ({"silence_threshold_db": -40}, "silence_threshold_db applies with trim_silence or max_pause_s"),
                    ({"trim_silence": False, "silence_threshold_db": -40}, "silence_threshold_db applies with trim_silence or max_pause_s")):
        with pytest.raises(ValueError, match=msg):
            parse_request("hi", **kw)


# ------------------------------------------------------------------------------- routing
def test_order_tuples():
    assert route.TRIM_ORDER == ("trim",) + engine.PASS_ORDER
    assert engine.STAGES == ("seam", "stretch", "resample", "flac")
    assert engine.LAUNCH_ORDER == ("seam", "loudness", "stretch", "resample", "flac")
    assert engine.PASS_ORDER == ("seam", "loudness", "stretch", "watermark", "resample", "flac")
    assert engine.FLOAT_STAGES == ("seam", "loudness", "stretch", "watermark")
    r = engine.SlotRoute()
    assert (r.trim, r.pause_blocks, r.thr) == (False, 0, float(THRESH)) and r.stages == ()
    assert [f.name for f in r.__dataclass_fields__.values()][-3:] == ["trim", "pause_blocks", "thr"]
    assert engine.SlotRoute(trim=True).stages == ("trim",) and engine.SlotRoute(pause_blocks=10).stages == ("trim",)
    assert engine.SlotRoute(thr=0.1).stages == ()  # a threshold alone trims nothing


def test_plans_without_a_trimming_slot_are_todays():
    def todays(routes):  # plan_pass as it was before the stage existed, over PASS_ORDER
        order = engine.PASS_ORDER
        paths = {b: tuple(s for s, o in zip(order, (r.segmented, r.loudness is not None, r.speed_q != 65536, r.watermark_gain > 0.0,
                                                    r.enc != 0, r.flac)) if o) for b, r in routes.items()}
        rows = {s: [b for b, p in paths.items() if s in p] for s in order}
        stages = [s for s in order if rows[s]]
        through = {s: [b for b, p in paths.items() if p and s not in p and order.index(p[-1]) > order.index(s)]
                   for s in engine.FLOAT_STAGES if rows[s]}
        source = {b: (p[-1] if p else None) for b, p in paths.items()}
        return stages, {s: rows[s] for s in stages}, through, source, [s for s in stages if s in source.values()]

    for c1, c2, loud, mark in itertools.product(COMBOS, COMBOS, (None, -20.0), (0.0, 0.05)):
        routes = {0: _route(*c1, mark=mark), 1: engine.SlotRoute(), 2: _route(*c2, loud=loud)}
        plan = engine.plan_pass(routes)
        assert (plan.stages, plan.rows, plan.through, plan.source, plan.host) == todays(routes)
        assert "trim" not in plan.stages and "trim" not in plan.rows and "trim" not in plan.through


def test_trimming_slots_beside_every_existing_combination():
    from dataclasses import replace

    for c1, c2 in itertools.product(COMBOS, COMBOS):
        batch = {0: _route(*c1), 1: replace(_route(*c2, mark=0.05), trim=True), 2: engine.SlotRoute(),
                 3: replace(_route(*c1, loud=-30.0), pause_blocks=11, thr=0.1)}
        plan = engine.plan_pass(batch)
        assert plan.stages[0] == "trim" and plan.stages == [s for s in route.TRIM_ORDER if any(s in r.stages for r in batch.values())]
        assert plan.rows["trim"] == [1, 3]
        for b, r in batch.items():
            assert plan.source[b] == (r.stages[-1] if r.stages else None)
            assert ("trim" in r.stages) == (b in (1, 3)) and (not r.stages or "trim" not in r.stages[1:])
        # slot 0 skips the stage: passed through when any stage serves it; the plain slot never is
        assert plan.through["trim"] == ([0] if batch[0].stages else [])
        for s in plan.through:
            want = [b for b, r in batch.items() if r.stages and s not in r.stages
                    and route.TRIM_ORDER.index(r.stages[-1]) > route.TRIM_ORDER.index(s)]
            assert plan.through[s] == want
        assert ("trim" in plan.host) == any(r.stages == ("trim",) for r in batch.values())
    only = engine.plan_pass({0: engine.SlotRoute(trim=True), 1: engine.SlotRoute()})
    assert only.stages == ["trim"] and only.host == ["trim"] and only.through == {"trim": []} and only.source == {0: "trim", 1: None}


def test_converter_makes_no_trim_stage_until_a_slot_asks(monkeypatch):
    import torch

    made = []

    class Stage:
        def __init__(self, device, batch):
            made.append("trim")

        def start_segments(self, slots, flags, trims, pauses, thrs):
            made.append(("start", list(slots), list(flags), list(trims), list(pauses), [float(t) for t in thrs]))

        def close(self):
            pass

    monkeypatch.setattr(route, "SilenceTrimmer", Stage)
    conv = engine.StreamConverter(torch.device("cpu"), 4, 1920)
    conv.reset_slots([0, 1], [None, None], [None, None])
    conv.reset_slots([0, 1], [None, None], [None, None], trim=[(False, 0, None), None])
    assert made == [] and conv.tr is None and not conv.converts(0) and conv.ends([0, 1]) == (False, False)
    conv.reset_slots([1], [None], [None], trim=[(True, 10, 0.1)])
    assert made == ["trim", ("start", [1], [FIRST | FINAL], [1], [10], [0.1])]
    assert conv.converts(1) and not conv.converts(0) and conv.ends([0, 1]) == (True, True) and conv.ends([0]) == (False, False)
    conv.reset_slots([1], [None], [None])
    assert made[-1] == ("start", [1], [engine.SEAM_OFF], [0], [0], [float(THRESH)]) and not conv.converts(1)
