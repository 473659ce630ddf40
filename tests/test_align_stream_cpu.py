"""Streamed character timestamps on the CPU: the numpy model ``align.StreamFit`` against the blocking ``align.fit``,
bit for bit, on planted rows (tests/align_stream_helpers.py); ``StreamAligner``'s parts; the refusals; the route on a stand-in."""
import base64
import json

import numpy as np
import pytest

import align_stream_helpers as hp
from smoltts_amd import align
from smoltts_amd.request import parse_request
from smoltts_amd.tokenizer import load_tokenizer


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ the model against fit
def test_the_result_does_not_depend_on_how_the_frames_are_cut_into_calls():
    m, s1 = hp.noisy(4)
    rows = np.stack([m, s1], axis=2)
    want = hp.model_trace(m, s1, 17, 3)[1]
    for step in (4, 8, 48):
        sf = align.StreamFit(17, 3)
        for f in range(0, 48, step):
            sf.push_rows(rows[f:f + step])
        assert np.array_equal(_bits(sf.finish(48)), _bits(want)), step


@pytest.mark.parametrize("lag", [1, 3, 6])
def test_each_start_is_fits_over_the_frames_seen_when_it_was_committed(lag):
    n = 17
    early = 0
    for seed in range(20):
        m, s1 = hp.noisy(seed)
        sf = align.StreamFit(n, lag)
        for f in range(m.shape[0]):
            before = sf.committed
            sf.push(m[f], s1[f])
            if sf.committed > before:
                ft = align.fit(m[:f + 1], s1[:f + 1], n)
                for i in range(before, sf.committed):
                    assert _bits(sf.starts[i]) == _bits(max(ft.starts[i], sf.starts[i - 1])), (seed, lag, f, i)
                    early += 1
    assert early > 20 * 8  # (the streams do commit early)


@pytest.mark.parametrize("H", [1, 2, 4])
def test_with_a_lag_of_the_whole_utterance_the_starts_are_fits(H):
    m, s1 = hp.noisy(3, H=H)
    trace, starts = hp.model_trace(m, s1, 17, 64)
    assert all(len(t) == 1 for t in trace)  # nothing commits early
    assert np.array_equal(_bits(starts), _bits(align.fit(m, s1, 17).starts))


@pytest.mark.parametrize("lag", [1, 2, 4, 6, 64])
def test_where_no_pooling_reaches_back_streamed_equals_blocking(lag):
    m, s1 = hp.ramp()
    assert np.array_equal(_bits(hp.model_trace(m, s1, 12, lag)[1]), _bits(align.fit(m, s1, 12).starts))


def test_an_outlier_behind_the_lag_is_frozen_out_and_one_inside_it_is_not():
    m, s1 = hp.ramp(outlier=True)
    F, ref = m.shape[0], align.fit(m, s1, 12).starts
    for lag in (6, 8, 64):
        assert np.array_equal(_bits(hp.model_trace(m, s1, 12, lag)[1]), _bits(ref)), lag
    got = hp.model_trace(m, s1, 12, 1)[1]
    assert (got != ref).any()  # the freeze is real: the blocking fit pools back across starts the stream had committed
    assert (np.diff(got) >= 0).all() and got[0] == 0.0 and (got >= 0).all() and (got <= F).all()
    assert (got != ref).sum() >= (hp.model_trace(m, s1, 12, 4)[1] != ref).sum() > 0  # a longer lag sees more


def test_weightless_rows_share_the_utterance_evenly_and_tiny_texts():
    m, s1 = hp.weightless()
    trace, starts = hp.model_trace(m, s1, 12, 6)
    assert all(len(t) == 1 for t in trace)
    assert np.array_equal(_bits(starts), _bits(np.arange(12) * (40 / 12))) and np.array_equal(_bits(starts), _bits(align.fit(m, s1, 12).starts))
    for rows in (hp.weightless(), hp.ramp(), hp.gaps()):
        assert hp.model_trace(*rows, 0, 6)[1].size == 0
        assert np.array_equal(hp.model_trace(*rows, 1, 6)[1], [0.0])
    m, s1 = hp.gaps()
    assert np.array_equal(_bits(hp.model_trace(m, s1, 12, 64)[1]), _bits(align.fit(m, s1, 12).starts))
    sf = align.StreamFit(12, 6)  # a stream cut short: what no block reaches ends at F, nothing lies behind it
    sf.push_rows(np.stack([m, s1], axis=2)[:10])
    cut = sf.finish(10)
    assert cut[-1] == 10.0 and (np.diff(cut) >= 0).all() and (cut <= 10).all()
    with pytest.raises(ValueError):
        sf.push(m[10], s1[10])


# ------------------------------------------------------------------------------------------------ parts
def _stream(text, m, s1, lag, speed=None, F=None, tok=None):
    """The parts of a stream of ``text`` over the planted rows, one ``update`` per frame, and the model's final starts."""
    tok = tok or load_tokenizer()
    ids = tok.encode(text).ids
    sf, al = align.StreamFit(len(ids), lag), align.StreamAligner(text, ids, tok, speed=speed)
    parts = []
    for f in range(m.shape[0]):
        sf.push(m[f], s1[f])
        parts.append(al.update(np.asarray(sf.starts)))
    F = m.shape[0] if F is None else F
    starts = sf.finish(F)
    parts.append(al.finish(starts, F * align.FRAME_S / (speed or 1.0)))
    return parts, al, starts, ids


class _Utf8Tokenizer:
    """One token per UTF-8 byte."""

    def encode(self, text):
        class E:
            ids = list(text.encode("utf-8"))
        return E

    def id_to_token(self, i):
        return None


def test_parts_concatenate_to_the_alignment_and_are_never_revised():
    text = "Hé, wörld: ok"  # multi-byte characters: their tokens share one interval
    n = len(text.encode("utf-8"))
    m, s1 = hp.ramp(n=n)
    tok = _Utf8Tokenizer()
    parts, al, starts, ids = _stream(text, m, s1, 2, tok=tok)
    assert len(ids) == n > len(text)
    handed = [p for p in parts if p is not None]
    assert len(handed) > 3 and parts[-1] is not None  # the stream does hand out parts before its end
    whole = al.alignment()
    assert whole.characters == list(text) == [c for p in handed for c in p.characters]
    assert whole.start_s[0] == 0.0 and whole.end_s[-1] == m.shape[0] * align.FRAME_S
    assert all(a <= b for a, b in zip(whole.start_s, whole.end_s)) and all(a <= b for a, b in zip(whole.start_s, whole.start_s[1:]))
    # each character spans its tokens' starts, in seconds: é is two tokens
    spans = align.token_spans(text, ids, tok)
    assert spans[1] == (1, 3)
    for k, (a, b) in enumerate(spans):
        assert whole.start_s[k] == starts[a] * align.FRAME_S
        assert whole.end_s[k] == (starts[b] * align.FRAME_S if b < n else m.shape[0] * align.FRAME_S)
    assert set(handed[0].to_json()) == {"characters", "character_start_times_seconds", "character_end_times_seconds"}
    # where streamed equals blocking in frames (the ramp), the concatenation is the blocking alignment
    blocking = align.align(text, ids, m, s1, tok)
    assert whole.start_s == blocking.start_s and whole.end_s == blocking.end_s
    with pytest.raises(ValueError):
        al.update(starts)


def test_a_dropped_character_stands_empty_where_it_would_be():
    text = "ab€cd€"  # the byte-level tokenizer has no token for what lies outside latin-1
    tok = load_tokenizer()
    m, s1 = hp.ramp(n=4)
    parts, al, starts, ids = _stream(text, m, s1, 2, tok=tok)
    assert len(ids) == 4
    whole = al.alignment()
    assert whole.characters == list(text)
    assert whole.start_s[2] == whole.end_s[2] == starts[2] * align.FRAME_S  # where c starts
    assert whole.start_s[5] == whole.end_s[5] == m.shape[0] * align.FRAME_S  # behind the last token: the end
    blocking = align.align(text, ids, m, s1, tok)
    assert whole.start_s == blocking.start_s and whole.end_s == blocking.end_s


def test_the_final_part_clamps_to_the_delivered_duration_at_a_speed():
    text = "speedy text"
    m, s1 = hp.ramp(n=len(text))
    F = m.shape[0]
    parts, al, starts, ids = _stream(text, m, s1, 6, speed=1.5)
    whole = al.alignment()
    total = F * align.FRAME_S / 1.5
    assert whole.end_s[-1] == total and max(whole.end_s) <= total and max(whole.start_s) <= total
    assert whole.start_s[3] == starts[3] * (align.FRAME_S / 1.5)  # nominal: frames over the speed
    # a stream that delivers fewer frames than it pushed (its budget): nothing lies behind what was delivered
    parts, al, starts, ids = _stream(text, m, s1, 6, speed=1.5, F=F - 8)
    whole = al.alignment()
    total = (F - 8) * align.FRAME_S / 1.5
    assert whole.end_s[-1] == total and max(p.end_s[-1] for p in parts[-1:] if p is not None) == total
    assert all(e <= total for e in parts[-1].end_s) and all(s <= total for s in parts[-1].start_s)
    with pytest.raises(ValueError):
        align.StreamAligner(text, ids, load_tokenizer()).finish(starts[:3], 1.0)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_a_request_with_live_timestamps():
    ok = parse_request("a text", stream=True)
    align.check_live_timestamps(ok, True, True)
    align.check_live_timestamps(parse_request("a text", stream=True, speed=1.5, output_format="pcm_16000", peak_limit_db=-1.0), True, True)
    with pytest.raises(ValueError, match="alignment_heads"):
        align.check_live_timestamps(ok, True, False)
    with pytest.raises(ValueError, match="use `timestamps`"):
        align.check_live_timestamps(parse_request("a text"), False, True)
    with pytest.raises(ValueError, match="timestamps"):
        align.check_live_timestamps(parse_request("a text", timestamps=True), True, True)
    for kw, word in ((dict(segment=True), "segment"), (dict(trim_silence=True), "trim_silence"), (dict(max_pause_s=0.5), "max_pause_s")):
        with pytest.raises(ValueError, match=word):
            align.check_live_timestamps(parse_request("a text", stream=True, **kw), True, True)
    with pytest.raises(ValueError, match="best_of"):
        align.check_live_timestamps(ok, True, True, takes=2)
    with pytest.raises(ValueError):  # the blocking option keeps its own refusal of a stream
        parse_request("a text", stream=True, timestamps=True)
    for bad in (0, 65, 6.0, True, None):
        with pytest.raises(ValueError):
            align.check_lag(bad)
    assert align.check_lag(1) == 1 and align.check_lag(64) == 64
    with pytest.raises(TypeError):  # it is no audio option: parse_request does not know it
        parse_request("a text", stream=True, live_timestamps=True)


def test_the_server_setting_and_the_abi_carry_the_lag_and_the_entries():
    from smoltts_amd import abi
    from smoltts_amd.server.settings import ServerSettings

    assert ServerSettings(checkpoint_dir="x").timestamp_lag_frames == 6
    for bad in (0, 65):
        with pytest.raises(ValueError):
            ServerSettings(checkpoint_dir="x", timestamp_lag_frames=bad)
    for name in ("bytes", "create", "destroy", "reset_slots", "push", "outputs"):
        assert "smoltts_align_fit_" + name in abi.SIGNATURES


# ------------------------------------------------------------------------------------------------ the route
class _FakeTTS:
    """A stand-in engine with ``SmolTTS.stream_with_timestamps``: one frame per character, the model over planted rows."""
    sampling_rate = 24000

    def __init__(self, heads):
        self.alignment_heads = heads
        self.calls = []

    def stream_with_timestamps(self, text, voice="heart", **kw):
        self.calls.append(kw)
        opts = parse_request(text, stream=True, **{k: v for k, v in kw.items() if k != "sampling"})
        align.check_live_timestamps(opts, True, bool(self.alignment_heads), getattr(kw.get("sampling"), "takes", 1))
        if len(text) > 1000:
            raise ValueError("prompt + max_new_tokens exceed max_seq_len")
        tok = load_tokenizer()
        ids = tok.encode(text).ids
        F = len(ids) + 2
        m, s1 = hp.rows_of(np.full((F, 1), 0.5), np.minimum(np.arange(F), len(ids) - 1))
        sf, al = align.StreamFit(len(ids), 2), align.StreamAligner(text, ids, tok, speed=kw.get("speed"))
        for f in range(F):
            sf.push(m[f], s1[f])
            part = al.update(np.asarray(sf.starts)) if f < F - 1 else al.finish(sf.finish(F), F * al.scale)
            chunk = np.full(1920, f / 100, np.float32)
            yield (chunk if "output_format" not in kw else (chunk * 32767).astype(np.int16)), part


def _client(heads, settings=None):
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from smoltts_amd.server.app import create_app

    tts = _FakeTTS(heads)
    return TestClient(create_app(tts, settings)), tts


def test_the_stream_route_answers_one_json_object_per_chunk():
    client, tts = _client([(0, 1)])
    text = "héllo"
    r = client.post("/v1/text-to-speech/3/stream/with-timestamps", json={"text": text})
    assert r.status_code == 200 and r.headers["content-type"].startswith("application/x-ndjson")
    objs = [json.loads(l) for l in r.text.splitlines()]
    assert len(objs) == len(text) + 2 and all(set(o) == {"audio_base64", "alignment", "normalized_alignment"} for o in objs)
    assert all(o["alignment"] == o["normalized_alignment"] for o in objs)
    assert any(o["alignment"] is None for o in objs) and objs[-1]["alignment"] is not None
    chars, st, en = [], [], []
    for o in objs:
        if o["alignment"] is not None:
            assert set(o["alignment"]) == {"characters", "character_start_times_seconds", "character_end_times_seconds"}
            chars += o["alignment"]["characters"]
            st += o["alignment"]["character_start_times_seconds"]
            en += o["alignment"]["character_end_times_seconds"]
    assert chars == list(text) and st[0] == 0.0 and en[-1] == pytest.approx(len(objs) * 0.08)
    assert all(a <= b for a, b in zip(st, en)) and all(a <= b for a, b in zip(st, st[1:]))
    audio = b"".join(base64.b64decode(o["audio_base64"]) for o in objs)
    assert np.array_equal(np.frombuffer(audio, np.float32)[::1920], np.arange(len(objs), dtype=np.float32) / 100)  # /stream's float32
    r16 = client.post("/v1/text-to-speech/3/stream/with-timestamps?output_format=pcm_16000", json={"text": text})
    assert r16.status_code == 200 and tts.calls[-1]["output_format"] == "pcm_16000" and r16.headers["x-sample-rate"] == "16000"
    assert len(base64.b64decode(json.loads(r16.text.splitlines()[0])["audio_base64"])) == 1920 * 2
    assert client.post("/v1/text-to-speech/3/stream/with-timestamps", json={}).status_code == 422


def test_the_stream_route_answers_501_without_heads_and_400_for_what_it_refuses():
    client, tts = _client(None)
    r = client.post("/v1/text-to-speech/3/stream/with-timestamps", json={"text": "abc"})
    assert r.status_code == 501 and "smoltts_amd.align rank" in r.json()["detail"] and not tts.calls
    client, tts = _client([(0, 1)])
    for body, word in (({"text": "abc", "trim_silence": True}, "trim_silence"), ({"text": "abc", "max_pause_s": 0.5}, "max_pause_s"),
                       ({"text": "abc", "temperature": 0.8, "best_of": 2}, "best_of"), ({"text": "x" * 2000}, "max_seq_len")):
        r = client.post("/v1/text-to-speech/3/stream/with-timestamps", json=body)
        assert r.status_code == 400 and word in r.json()["detail"], (body, r.status_code, r.text)
    client, tts = _client([(0, 1)], {"long_text": "segment"})  # a server that segments long texts speaks the request as one utterance
    assert client.post("/v1/text-to-speech/3/stream/with-timestamps", json={"text": "One. Two."}).status_code == 200
    assert "segment" not in tts.calls[-1]
