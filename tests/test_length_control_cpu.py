"""Per-request length control without a GPU: the option's validation and resolution, the seconds spelling, the bounds from the text
length (per segment of a plan), the numpy model of the patch, the finish reason, the route bodies, the entries a slot's tenants
write, and the ABI's new struct and symbols."""
import ctypes as C
import math

import numpy as np
import pytest

from smoltts_amd import abi
from smoltts_amd.config import (FRAMES_PER_SECOND, GenerationSettings, RequestSampling, finish_reason, length_bounds,
                                merge_finish_reasons, min_frames_from)


# ---------------------------------------------------------------------------------------------------- the option
def test_request_sampling_ranges():
    for ok in (dict(min_frames=0), dict(min_frames=1024), dict(eos_bias=-100), dict(eos_bias=100.0), dict(eos_bias=0), dict(min_frames=7, eos_bias=2.5)):
        RequestSampling(**ok)
    for bad in (dict(min_frames=-1), dict(min_frames=1025), dict(min_frames=3.0), dict(min_frames=True), dict(eos_bias=100.5),
                dict(eos_bias=-101), dict(eos_bias=float("nan")), dict(eos_bias=float("inf")), dict(eos_bias="3"), dict(eos_bias=True)):
        with pytest.raises(ValueError):
            RequestSampling(**bad)
    with pytest.raises(ValueError):
        GenerationSettings(min_frames=2000)
    with pytest.raises(ValueError):
        GenerationSettings(eos_bias=float("nan"))


def test_length_on_and_resolve():
    assert not RequestSampling().length_on and not RequestSampling(min_frames=0, eos_bias=0.0).length_on
    assert RequestSampling(min_frames=1).length_on and RequestSampling(eos_bias=-0.5).length_on
    gs = GenerationSettings.greedy()
    off = RequestSampling().resolve(gs)
    assert (off.min_frames, off.eos_bias) == (0, 0.0) and not off.length_on and isinstance(off.min_frames, int)
    defaults = GenerationSettings(default_temp=0.0, default_fast_temp=0.0, min_frames=25, eos_bias=-1.5)
    r = RequestSampling().resolve(defaults)
    assert (r.min_frames, r.eos_bias) == (25, -1.5) and r.length_on
    own = RequestSampling(min_frames=0, eos_bias=4.0).resolve(defaults)  # a request's explicit 0 switches the default off
    assert (own.min_frames, own.eos_bias) == (0, 4.0)
    assert own.resolve(defaults) == own  # resolving a resolved entry changes nothing
    # the other fields are untouched by the new ones
    a, b = RequestSampling(temperature=0.7, seed=5).resolve(gs), RequestSampling(temperature=0.7, seed=5, min_frames=3).resolve(gs)
    assert (a.temperature, a.fast_temperature, a.min_p, a.seed, a.top_p, a.top_k) == (b.temperature, b.fast_temperature, b.min_p, b.seed, b.top_p, b.top_k)
    assert a != b


def test_min_duration_spelling():
    assert FRAMES_PER_SECOND == 12.5
    assert min_frames_from(None, None) is None and min_frames_from(9, None) == 9
    assert min_frames_from(None, 0) == 0 and min_frames_from(None, 1.0) == 13 and min_frames_from(None, 0.08) == 1
    assert min_frames_from(None, 2) == 25 and min_frames_from(None, 0.16) == 2 and min_frames_from(None, 81.92) == 1024
    for s in (0.3, 1.7, 10.01):
        assert min_frames_from(None, s) == math.ceil(s * 12.5)
    for bad in ((3, 1.0), (None, -0.1), (None, float("nan")), (None, float("inf")), (None, 82.0), (None, True), (None, "1")):
        with pytest.raises(ValueError):
            min_frames_from(*bad)


# ---------------------------------------------------------------------------------------------------- bounds from the text
def test_length_bounds_arithmetic():
    gs = GenerationSettings.greedy()
    base = RequestSampling().resolve(gs)
    text = "héllo wörld"  # 11 characters, 13 bytes
    assert len(text.encode()) == 13
    assert length_bounds(text, base, 100) == (base, 100) and length_bounds(text, base, 100)[0] is base  # both off: untouched
    s, cap = length_bounds(text, base, 100, min_frames_per_byte=0.5, max_frames_per_byte=2.0)
    assert cap == 26 and s.min_frames == 6  # ceil(13 * 2), floor(13 * 0.5)
    s, cap = length_bounds(text, base, 20, max_frames_per_byte=2.0)
    assert cap == 20 and s is base  # the request's own cap is the smaller
    s, cap = length_bounds("", base, 20, min_frames_per_byte=1.0, max_frames_per_byte=2.0)
    assert cap == 1 and s.min_frames == 0  # at least 1; the minimum stays below the cap
    s, cap = length_bounds(text, RequestSampling(min_frames=9).resolve(gs), 100, min_frames_per_byte=0.5)
    assert s.min_frames == 9 and cap == 100  # the request's own minimum is the larger
    s, cap = length_bounds(text, RequestSampling(min_frames=9).resolve(gs), 100, min_frames_per_byte=1.5)
    assert s.min_frames == 19
    s, cap = length_bounds(text, base, 10, min_frames_per_byte=3.0)
    assert s.min_frames == 9  # never above the cap - 1
    s, cap = length_bounds(text, base, 100, min_frames_per_byte=3.0, max_frames_per_byte=0.5)
    assert cap == 7 and s.min_frames == 6
    s, cap = length_bounds("x" * 5000, base, 4000, min_frames_per_byte=1.0)
    assert s.min_frames == 1024  # the public range
    assert s.eos_bias == base.eos_bias and s.seed == base.seed and s.temperature == base.temperature


def test_segments_of_a_plan_get_their_own_bounds():
    from smoltts_amd.longform import GrowingPlan, SegmentOptions, SegmentPlan

    text = "Short one. " + "A much longer second sentence that goes on for quite a while before it ends. " + "End."
    plan = SegmentPlan.create(text, SegmentOptions(max_bytes=80))
    assert plan is not None and len(plan.segs) == 3
    base = RequestSampling(temperature=0.7, seed=3, min_frames=4).resolve(GenerationSettings.greedy())
    got = []
    for k, seg in enumerate(plan.segs):
        s, cap = plan.length_bounds(k, plan.sampling(k, base), 64, min_frames_per_byte=0.25, max_frames_per_byte=0.75)
        n = len(seg.text.encode("utf-8"))
        assert cap == max(1, min(64, math.ceil(n * 0.75))) and s.min_frames == min(max(4, math.floor(n * 0.25)), cap - 1), (k, n)
        assert s.seed == plan.sampling(k, base).seed  # the segment's seed stays its own
        got.append((s.min_frames, cap))
    assert len(set(got)) == 3 and got[1][0] > got[0][0] >= 4 and got[1][1] > got[0][1] > got[2][1]
    # without the ratios every segment keeps the request's entry and cap
    assert all(plan.length_bounds(k, base, 64) == (base, 64) for k in range(3))
    grow = GrowingPlan(SegmentOptions(max_bytes=80))
    grow.extend(plan.segs[:2])
    assert grow.length_bounds(1, base, 64, 0.25, 0.75) == plan.length_bounds(1, base, 64, 0.25, 0.75)


def test_facade_bounds_give_a_session_wide_call_its_entry():
    """``SmolTTS._bounded``: a call without ``sampling=`` whose text turns a minimum on gets the resolved entry that carries it (the
    length control exists in slot mode only), from the plain text or from the plan's segment."""
    from types import SimpleNamespace

    from smoltts_amd import SmolTTS
    from smoltts_amd.longform import SegmentOptions, SegmentPlan

    gs = GenerationSettings(default_temp=0.0, default_fast_temp=0.0, max_new_tokens=50, seed=17)
    me = SimpleNamespace(min_frames_per_byte=0.5, max_frames_per_byte=None, _bounds_on=True, _max_new=lambda s: s.max_new_tokens)
    st, entry = SmolTTS._bounded(me, "twenty bytes of text.", gs, None)
    assert st.max_new_tokens == 50 and st.min_frames == 10 and [e.min_frames for e in entry] == [10] and entry[0].seed == 17
    given = [RequestSampling(temperature=0.6, seed=3, min_frames=12).resolve(gs)]
    st, entry = SmolTTS._bounded(me, "twenty bytes of text.", gs, given)
    assert st.min_frames == 0 and entry[0].min_frames == 12 and entry[0].seed == 3  # the request's own is the larger
    me.min_frames_per_byte, me.max_frames_per_byte = None, 1.0
    st, entry = SmolTTS._bounded(me, "twenty bytes of text.", gs, None)
    assert st.max_new_tokens == 21 and entry is None  # only the cap: the call stays session-wide
    plan = SegmentPlan.create("Short one. A much longer second sentence that goes on for quite a while before it ends. End.", SegmentOptions(max_bytes=80))
    me.min_frames_per_byte = 0.25
    got = [SmolTTS._bounded(me, "ignored where a plan is given", gs, None, plan, k) for k in range(3)]
    assert [(st.min_frames, st.max_new_tokens, None if e is None else e[0].min_frames) for st, e in got] == \
        [(m, c, m or None) for m, c in ((lambda n: (min(math.floor(n * 0.25), min(50, n) - 1), min(50, n)))(len(s.text.encode())) for s in plan.segs)]
    me._bounds_on = False
    assert SmolTTS._bounded(me, "x", gs, None) == (gs, None)


# ---------------------------------------------------------------------------------------------------- the numpy model
def test_length_patch():
    from smoltts_amd.sampling import length_patch

    x = np.array([0.25, -1.5, 3.0, 2.75], np.float32)
    for kw in (dict(), dict(min_frames=0, eos_bias=0.0), dict(min_frames=5)):  # off, or the minimum already reached
        out = length_patch(x, 3, 5, **kw)
        assert out.dtype == np.float32 and np.array_equal(out, x) and out is not x
    assert np.array_equal(length_patch(x, 3, 4, min_frames=5), np.array([0.25, -1.5, 3.0, -np.inf], np.float32))
    assert np.array_equal(length_patch(x, 3, 0, min_frames=1, eos_bias=1e4), np.array([0.25, -1.5, 3.0, -np.inf], np.float32))
    assert np.array_equal(length_patch(x, 3, 9, min_frames=1, eos_bias=0.5), np.array([0.25, -1.5, 3.0, 3.25], np.float32))
    assert int(np.argmax(length_patch(x, 3, 9, eos_bias=0.25))) == 2  # a tie: the first index
    assert int(np.argmax(length_patch(x, 3, 9, eos_bias=0.5))) == 3
    # one rounded fp32 add, not a float64 one
    y = np.array([1.0, 1e-3], np.float32)
    want = np.float32(np.float32(1e-3) + np.float32(1e4))
    assert length_patch(y, 1, 0, eos_bias=1e4)[1] == want and float(want) != float(np.float32(1e-3)) + 1e4
    assert np.array_equal(x, np.array([0.25, -1.5, 3.0, 2.75], np.float32))  # the input is never written


def test_finish_reason():
    assert finish_reason([5, 6, 7, 99], 99) == "stop"
    assert finish_reason([5, 99, 7], 99) == "length"  # an earlier <|im_end|> (stop_on_eos off) does not count
    assert finish_reason(np.array([5, 6], np.int32), 99) == "length" and finish_reason([], 99) == "length"
    assert finish_reason(np.array([99], np.int64), 99) == "stop"
    assert merge_finish_reasons(["stop", "stop"]) == "stop" and merge_finish_reasons(["stop", "length", "stop"]) == "length"
    assert merge_finish_reasons(["stop"]) == "stop"


# ---------------------------------------------------------------------------------------------------- what a slot's tenants write
class _Recorder:
    def __init__(self):
        self.filtered_slots, self.length_slots, self.calls = set(), set(), []

    def set_slot_sampling(self, *a):
        self.calls.append(("sampling", a[0]))

    def set_slot_filters(self, *a):
        self.calls.append(("filters", *a))

    def set_slot_length(self, slots, min_frames, eos_bias):
        self.calls.append(("length", list(slots), list(min_frames), list(eos_bias)))
        for b, m, x in zip(slots, min_frames, eos_bias):
            (self.length_slots.add if (m > 0 or x != 0) else self.length_slots.discard)(b)


def test_a_tenant_without_the_option_writes_an_off_entry():
    from smoltts_amd.generate import _apply_slot_sampling, resolve_sampling

    gs = GenerationSettings.greedy()
    plain, on = RequestSampling().resolve(gs), RequestSampling(min_frames=5, eos_bias=-2.0).resolve(gs)
    s = _Recorder()
    _apply_slot_sampling(s, [0, 1, 2], [plain, on, plain])
    assert [c for c in s.calls if c[0] == "length"] == [("length", [1], [5], [-2.0])]  # only where one is on
    s.calls.clear()
    _apply_slot_sampling(s, [1, 2], [plain, RequestSampling(eos_bias=1.0).resolve(gs)])  # slot 1 is recycled: cleared
    assert [c for c in s.calls if c[0] == "length"] == [("length", [1, 2], [0, 0], [0.0, 1.0])] and s.length_slots == {2}
    s.calls.clear()
    _apply_slot_sampling(s, [0, 1], [plain, plain])
    assert not [c for c in s.calls if c[0] == "length"]  # nothing on, nothing left over: no upload
    # the façade's session-wide mode stays what it was; settings that turn the control on put every utterance in slot mode
    assert resolve_sampling(None, gs, 2) is None
    r = resolve_sampling(None, GenerationSettings(default_temp=0.0, default_fast_temp=0.0, min_frames=4, seed=11), 2)
    assert [x.min_frames for x in r] == [4, 4] and r[0].seed == 11


# ---------------------------------------------------------------------------------------------------- route bodies and settings
def test_route_bodies():
    pytest.importorskip("fastapi")
    from pydantic import ValidationError

    from smoltts_amd.server.app import CreateSpeechRequest, SpeechRequest, StreamInputOptions, _finish_headers

    for cls, text in ((SpeechRequest, {"input": "x"}), (CreateSpeechRequest, {"text": "x"}), (StreamInputOptions, {})):
        assert cls.model_validate(text).request_sampling() is None
        s = cls.model_validate({**text, "min_frames": 12, "eos_bias": -3}).request_sampling()
        assert (s.min_frames, s.eos_bias, s.temperature, s.seed) == (12, -3.0, None, None) and s.length_on
        s = cls.model_validate({**text, "min_duration_s": 1.0, "temperature": 0.5}).request_sampling()
        assert (s.min_frames, s.eos_bias, s.temperature) == (13, None, 0.5)
        assert cls.model_validate({**text, "min_duration_s": 0}).request_sampling().min_frames == 0
        assert cls.model_validate({**text, "eos_bias": 0}).request_sampling().eos_bias == 0.0
        for bad in ({"min_frames": -1}, {"min_frames": 1025}, {"min_frames": 2.5}, {"min_duration_s": -1}, {"min_duration_s": 82},
                    {"eos_bias": 101}, {"eos_bias": -100.5}, {"eos_bias": "loud"}, {"min_frames": 3, "min_duration_s": 0.2}):
            with pytest.raises(ValidationError):
                cls.model_validate({**text, **bad})
    assert _finish_headers({}) == {} and _finish_headers({"finish_reason": "length"}) == {"X-Finish-Reason": "length"}


def test_server_settings():
    pytest.importorskip("pydantic")
    from pydantic import ValidationError

    from smoltts_amd.server.settings import GenerationBlock, ServerSettings

    st = ServerSettings(checkpoint_dir="/nowhere")
    assert st.min_frames_per_byte is None and st.max_frames_per_byte is None  # no default ratio
    assert (st.generation.min_frames, st.generation.eos_bias) == (0, 0.0)
    gs = st.generation.to_settings()
    assert (gs.min_frames, gs.eos_bias) == (0, 0.0) and not RequestSampling().resolve(gs).length_on
    st = ServerSettings(checkpoint_dir="/nowhere", min_frames_per_byte=0.4, max_frames_per_byte=1.5, generation={"min_frames": 6, "eos_bias": -1})
    gs = st.generation.to_settings()
    assert (st.min_frames_per_byte, st.max_frames_per_byte, gs.min_frames, gs.eos_bias) == (0.4, 1.5, 6, -1.0)
    for bad in (dict(min_frames_per_byte=-1), dict(max_frames_per_byte=float("nan")), dict(generation={"min_frames": 1025}),
                dict(generation={"eos_bias": 1000})):
        with pytest.raises(ValidationError):
            ServerSettings(checkpoint_dir="/nowhere", **bad)
    assert GenerationBlock().to_settings() == GenerationBlock(min_frames=0, eos_bias=0).to_settings()


def test_model_only_core_takes_the_ratios_from_the_settings():
    pytest.importorskip("fastapi")
    from smoltts_amd.server.app import TTSCore

    class Model:
        min_frames_per_byte = None
        max_frames_per_byte = None

    m = Model()
    TTSCore(m, {"min_frames_per_byte": 0.5})
    assert m.min_frames_per_byte == 0.5 and m.max_frames_per_byte is None
    m2 = Model()
    TTSCore(m2, {"max_frames_per_byte": 2}, scheduler=object())  # behind a scheduler the bounds are the scheduler's
    assert m2.max_frames_per_byte is None


# ---------------------------------------------------------------------------------------------------- ABI 9
def test_abi_struct_and_symbols():
    assert abi.ABI_VERSION == 9 and abi.LENGTH_MAX_FRAMES == 2**30
    S = abi.SlotLength
    assert C.sizeof(S) == 16 and S in abi.STRUCTS
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("min_frames", 0, 4), ("eos_bias", 4, 4), ("reserved", 8, 8)]
    assert S._fields_[0][1] is C.c_int32 and S._fields_[1][1] is C.c_float
    assert abi.SIGNATURES["smoltts_session_set_slot_length"] == (abi.INT, "p p i p p p")
    assert abi.SIGNATURES["smoltts_k_sample_rows_length"] == (abi.INT, "p i i q p p p p p p i i p p")
    # additive: the entries it sits beside are what they were
    assert abi.SIGNATURES["smoltts_k_sample_rows_filtered"] == (abi.INT, "p i i q p p p p p i p p")
    assert abi.SIGNATURES["smoltts_session_set_slot_filters"] == (abi.INT, "p p i p p p p p")
    assert C.sizeof(abi.SlotSampling) == 24 and C.sizeof(abi.SlotFilters) == 32
    lib = abi.load_library()  # (the built library: its version and the two exports)
    assert lib.smoltts_abi_version() == 9
    assert hasattr(lib, "smoltts_session_set_slot_length") and hasattr(lib, "smoltts_k_sample_rows_length")


def test_slot_length_table_layout():
    torch = pytest.importorskip("torch")
    from smoltts_amd import ops

    t = ops.slot_length_table([0, 7, 2**30], [0.0, -3.5, 1e4], device="cpu")
    assert t.dtype == torch.uint8 and t.numel() == 48
    raw = t.numpy().tobytes()
    rows = [abi.SlotLength.from_buffer_copy(raw[16 * i: 16 * i + 16]) for i in range(3)]
    assert [(r.min_frames, r.eos_bias, list(r.reserved)) for r in rows] == [(0, 0.0, [0, 0]), (7, -3.5, [0, 0]), (2**30, 1e4, [0, 0])]
